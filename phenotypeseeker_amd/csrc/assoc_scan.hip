// a4-a7: the chi2 scan KERNELS over the bit-packed presence matrix, and nothing else: every chi2 kernel, the weighted
// finalize pass, their device helpers, their compile-time tuning macros, and the launch functions that instantiate them
// (launch_chi2_any, chi2_launch.h, is how chi2_driver.hip reaches them).  What the host decides about a scan is
// chi2_plan.h; the driver and the exported calls are chi2_driver.hip.  bench.py quotes a committed HBM traffic figure only
// for the sha256 of THIS file, the scan kernel's source: host-side edits live elsewhere and leave the figure standing.
//
// chi2_scan_kernel   replaces phenotypes.get_kmers_tested / conduct_chi_squared_test and helpers
//                    (modeling.py:677-714, :759-858)
// ttest_scan_kernel  (ttest_scan.hip) replaces conduct_t_test / get_samples_distribution_for_ttest (:716-757)
// chi2_scan_kernel_cx  the unweighted chi2 scan over the exception-coded copy of the matrix (presence_compact.hip), when
//                      there is one: same survivors, a third of the bytes at config 2
// chi2_scan_kernel_cx_side, ..._side_pc, ..._side_idx  the same scan when no slot row can pass: the side matrix alone, through
//                      its popcounts, or -- few feasible rows -- through the encoder's index of its rows by popcount
//
// Layout: bits[M][wpr] u64, wpr even, so a row is wpr/2 16-byte chunks.  G = next power of two
// >= wpr/2 lanes own one row; every lane issues one 16-byte load per row (global_load_dwordx4,
// consecutive lanes -> consecutive addresses), popcounts its two words against the phenotype
// masks and the group combines with xor-shuffles.  A wave covers 64/G rows per step and keeps
// UNROLL steps of loads in flight (stream_rows, scan_common.h).  HBM-read bound: 1 bit per k-mer x sample cell; no LDS, no MFMA.
// Up to 64 samples (r04; the reference's own example set has ~30) a row is ONE u64 (wpr = 1) and a lane's
// 16-byte load holds two rows: the kernels' G = 0 instantiations ("half a lane per row", 128 rows per wave
// step); masks and per-sample tables stay padded to a whole 16-byte chunk (cpr = 1).
//
// Exactness: the 2x2 table is integer (unit weights), and the statistic is evaluated with the
// reference's own operation order in IEEE double (this file is compiled with -ffp-contract=off),
// so round(chi2, 2) and "%.2E" % p come out string-identical.  The expensive exact evaluation only
// runs on rows that a division-free test T*(ad-bc)^2 >= thr*R1*R0*K1*K0*(1-1e-9) cannot rule out
// (chi2_candidate, chi2_plan.h: the rule as the dense kernel and the host's plans call it; the exception-coded kernels
// below restate it by hand).
#include "chi2_launch.h"

namespace {

// modeling.py:773-794 in the reference's operation order.
__device__ __forceinline__ double chi2_exact(double A, double B, double C, double D)
{
    const double w_pheno = A + B, wo_pheno = C + D, w_kmer = A + C, wo_kmer = B + D;
    const double total = w_pheno + wo_pheno;
    const double e0 = (w_pheno * w_kmer) / total, e1 = (w_pheno * wo_kmer) / total;
    const double e2 = (wo_pheno * w_kmer) / total, e3 = (wo_pheno * wo_kmer) / total;
    double stat = 0.0, d;
    d = A - e0; stat += (d * d) / e0;
    d = B - e1; stat += (d * d) / e1;
    d = C - e2; stat += (d * d) / e2;
    d = D - e3; stat += (d * d) / e3;
    return stat;
}

// The chi2 decision, once: statistic, p and the keep rule from the four cells.  The scan kernels append what is kept to
// a reserved slot (chi2_decide); chi2w_finalize_kernel compacts on the answer (`valid`: the lane holds a candidate) and
// stores to the compacted position.  The operation order is the reference's and must not move.
__device__ __forceinline__ bool chi2_keep(const ScanCuts &K, double A, double B, double C, double D, double &stat, double &p, bool valid = true)
{
    stat = chi2_exact(A, B, C, D);
    p = exp(-0.5 * stat);  // chi2.sf(stat, df = 2), modeling.py:782-792
    return valid && ((K.omit_B && p < K.pcut) || (p < K.pcut_bonf));  // modeling.py:795
}

__device__ __forceinline__ void chi2_store(const ScanSink &S, uint64_t idx, uint64_t row, double stat, double p, int n_w)
{
    S.res_row[idx] = row;
    S.res_stat[idx] = stat;
    S.res_p[idx] = p;
    S.res_nw[idx] = n_w;
}

__device__ __forceinline__ void chi2_decide(const ScanArgs &P, uint64_t row, double A, double B, double C, double D, int n_w)
{
    double stat, p;
    if (chi2_keep(P.cut, A, B, C, D, stat, p)) chi2_store(P.sink, reserve_slot(P.sink), row, stat, p, n_w);
}

// chi2_scan_kernel MODE 0 from the two class counts of a row (I: int, or uint32_t where they come as popcounts -- the
// conversions are then the candidate rule's own)
template <class I>
__device__ __forceinline__ void chi2_evaluate(const ScanCuts &K, const ScanSink &S, uint64_t row, I a, I c)
{
    double stat, p;
    if (chi2_keep(K, (double)a, (double)(K.n1 - (int)a), (double)c, (double)(K.n0 - (int)c), stat, p)) chi2_store(S, reserve_slot(S), row, stat, p, (int)(a + c));
}

// MODE 0: unit weights, the exact evaluation in line -- the usual case, where almost no row passes the pre-test.
// MODE 1: GSC weights: rows that pass the frequency filter are queued per wave and handled 64 at a time, one per lane.
// MODE 2: unit weights, rows that pass the pre-test are queued the same way: a scan with many survivors
//         (--omit_B_correction keeps ~pvalue of all rows) then evaluates 64 of them per pass instead of one or two
//         lanes of a wave at a time.  Same formulas, same results as MODE 0 (the host picks, see pick_chi2_mode).
template <int G, int MODE, bool LUT = false, bool F32 = false>
__global__ __launch_bounds__(LUT ? SC_LUT_THREADS : SC_THREADS) void chi2_scan_kernel(const ScanArgs P)
{
    constexpr bool WEIGHTED = MODE == 1, QUEUED = MODE != 0;
    constexpr bool HALF = G == 0;          // 8-byte rows, two per load
    constexpr int THREADS = sc_threads<G, LUT>(), UNR = sc_unroll<G, LUT>();
    if (!WEIGHTED) stamp_scan_start(P.sink);   // (the weighted scan is two kernels, timed by events)
    __shared__ uint64_t s_qrow[QUEUED ? THREADS / 64 : 1][QUEUED ? rq_cap(G, UNR) : 1];
    __shared__ int2 s_qval[QUEUED ? THREADS / 64 : 1][QUEUED ? rq_cap(G, UNR) : 1];
    extern __shared__ __attribute__((aligned(16))) double s_lut[];   // LUT: the nibble table of row_moments_lut / the six-bit f32 table
    if (LUT && F32) load_lut(s_lut, reinterpret_cast<const double *>(P.lut6), (int)(lut6_bytes(P.cpr, 2) / 8), THREADS);
    else if (LUT) load_lut(s_lut, P.lut, P.c_lut * 32 * 16 * 2, THREADS);
    const int lane = threadIdx.x & 63;
    const int g = lane & (sc_lanes(G) - 1);
    RowMasks<2> mk = {{0, 0}, {0, 0}, {P.m1, P.m0}};   // [0]: phenotype 1, [1]: phenotype 0
    if (g < P.cpr) {
        if (P.inline_masks) { mk.a[0] = P.m1_inl[2 * g]; mk.b[0] = P.m1_inl[2 * g + 1]; mk.a[1] = P.m0_inl[2 * g]; mk.b[1] = P.m0_inl[2 * g + 1]; }
        else { mk.a[0] = P.m1[2 * g]; mk.b[0] = P.m1[2 * g + 1]; mk.a[1] = P.m0[2 * g]; mk.b[1] = P.m0[2 * g + 1]; }
    }
    RowQueue Q = {s_qrow[QUEUED ? (threadIdx.x >> 6) : 0], s_qval[QUEUED ? (threadIdx.x >> 6) : 0], 0};
    // `cnt` queued rows, one per lane.  Weighted: class weight sums in sample order, then the same pre-test / exact
    // statistic / keep rule as the unweighted path.  MODE 2: the row has passed the pre-test; (a, c) came with it.
    // (Queueing costs the usual sparse case 4 % -- r01 A/B on cfg 2: 110.7 vs 115.2 us -- hence MODE 0.)
    auto process = [&](int cnt) {
        const bool act = lane < cnt;
        const uint64_t r = Q.row[act ? lane : 0];
        const int2 qv = Q.val[act ? lane : 0];
        int r_nw = qv.x;
        double A, B, C, D;
        if (WEIGHTED && F32) {
            // f32 class-weight sums (A, C may be off by e0, e1): an UPPER bound of the statistic decides who is a candidate.
            // det = AD - BC = A W0 - C W1 is linear in the two sums; the column totals shrink by the error
            double ws[2];
            row_moments_f32<2, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, reinterpret_cast<const float *>(s_lut), ws);
            const double T = P.W1 + P.W0, err = P.e0 + P.e1;
            const double det = fabs(ws[0] * P.W0 - ws[1] * P.W1) + (P.e0 * P.W0 + P.e1 * P.W1);
            const double K1 = (ws[0] + ws[1]) - err, K0 = (T - (ws[0] + ws[1])) - err;
            const bool cand = !(K1 > 0.0 && K0 > 0.0) || !(T * det * det < P.cut.thr * P.W1 * P.W0 * K1 * K0 * (1.0 - 1e-9));
            if (act && cand) append_candidate(P.sink, r, r_nw);
            return;
        } else if (WEIGHTED) {
            double ws[2];
            if (LUT) row_moments_mixed<2, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, P.c_lut, s_lut, (cdptr)P.tab, ws);
            else row_moments<2, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, (cdptr)P.tab, ws);
            A = ws[0]; B = P.W1 - ws[0]; C = ws[1]; D = P.W0 - ws[1];
            const double R1 = A + B, R0 = C + D, K1 = A + C, K0 = B + D, T = R1 + R0;
            const double det = A * D - B * C;
            const double lhs = T * det * det, rhs = P.cut.thr * R1 * R0 * K1 * K0;
            // candidates only: chi2w_finalize_kernel gives them the reference's own cells and decides (the sums here
            // associate differently, ~1e-15: hence the 1e-9 margin)
            if (act && !(lhs < rhs * (1.0 - 1e-9))) append_candidate(P.sink, r, r_nw);
            return;
        } else {
            if (!act) return;
            A = (double)qv.x; B = (double)(P.cut.n1 - qv.x); C = (double)qv.y; D = (double)(P.cut.n0 - qv.y);
            r_nw = qv.x + qv.y;
        }
        chi2_decide(P, r, A, B, C, D, r_nw);
    };

    auto on_row = [&](uint64_t row, const uint32_t (&cnt)[2], bool lead) {
        const uint32_t a = cnt[0], c = cnt[1];
        if (WEIGHTED) {
            const bool freq_ok = chi2_freq_ok(P.cut, a, c, row < P.M);
            Q.n = queue_rows(freq_ok && lead, row, make_int2((int)(a + c), 0), Q.row, Q.val, Q.n, lane);
            return;
        }
        const bool cand = chi2_candidate(P.cut, a, c, row < P.M, lead);
        if (MODE == 2) {
            Q.n = queue_rows(cand, row, make_int2((int)a, (int)c), Q.row, Q.val, Q.n, lane);
            return;
        }
        if (cand) chi2_evaluate(P.cut, P.sink, row, a, c);
    };
    if constexpr (QUEUED) stream_rows<G, LUT>(P, mk, Q, on_row, process);
    else stream_rows<G, LUT>(P, mk, Q, on_row, NoQueue());
    if (!WEIGHTED) publish_segment(P.sink);   // weighted: chi2w_finalize_kernel publishes
}

// ---- the unweighted scan over the exception-coded rows (presence_compact.hip) ------------------------------------------
// One lane per row: a lane's 16-byte load holds two slots, so a wave instruction reads 1 KB.  A slot's header gives e and
// whether the exceptions are the present or the absent samples; the class table in LDS (1 = case, 0x100 = control, 0 = NA)
// summed over the e indices gives (a', c') with a', c' <= 7, hence (a, c) = (a', c') or (n1 - a', n0 - c').  A slot row's
// table therefore lies in one of the two 8 x 8 corners of the (a, c) plane, and whether it is a candidate -- frequency
// filter and the division-free pre-test -- is one bit of the two corner words the host filled for this scan (cx_plan, through
// chi2_candidate, the dense kernel's rule); candidates take chi2_scan_kernel's MODE 0 path (chi2_exact, exp, keep rule), so
// stat and p are the dense kernel's bits.  A header class (e, base) none of whose reachable corner points is a candidate
// is dropped on the header byte (X.class_mask); when NO class is feasible -- every Bonferroni cut-off of a real run: a row
// of at most 7 exceptions cannot reach the statistic -- the host launches no slot workgroup and the slots are not read.
// The rows with more than CX_MAX_E exceptions are a side matrix of dense rows that the last workgroups of the SAME launch
// scan as chi2_scan_kernel's MODE 0 does (CPR 16-byte chunks per row, one lane each; the candidate rule
// restated by hand, see SideRows), reporting their original row ids: a second launch would add a kernel boundary to every step.
#ifndef PSK_CX_NT
#define PSK_CX_NT 0   // plain loads: 57.4 us against 60.7 us with the nontemporal hint at config 2
#endif
#ifndef PSK_CX_SIDE_NT
#define PSK_CX_SIDE_NT 1   // nontemporal hint on the side matrix: lower in five of six pairs of the r13 table (docs/NOTEBOOK.md), also re-read launch after launch
#endif
#ifndef PSK_CX_PC_NT
#define PSK_CX_PC_NT 0   // nontemporal hint on the popcount loads
#endif
// (the unrolls and grid multiples, which the launch shapes depend on, are chi2_plan.h's)

// The rows of the side matrix, once: UNR wave steps of 64 / CPR rows from step s0 on, one lane per 16-byte chunk.
// load() issues the batch's loads; evaluate() is chi2_scan_kernel MODE 0's on_row on what came back -- popcounts against
// the lane's mask words, the sum over the row's CPR lanes, the candidate rule, then the exact decision -- and reports a
// survivor under its original row id.  Both are called by whole waves (the CPR = 2 shuffle).
// The candidate rule is RESTATED BY HAND here and in PcRows: the same operations in the same order as chi2_candidate
// (chi2_plan.h), but nothing structural ties them to it -- the GPU tests that cross these kernels with the dense one bit
// for bit are what holds them together.  Called through the function, and with the tail and the sweep loop shared
// between the two structs, the compiler gave these kernels other registers than the parent's where a refactor has to leave
// them equal (chi2_scan_kernel_cx_side_pc<2>: 101 VGPRs against 99, 6 SGPR spills against 4; ..._cx_side<2>: 92 against
// 96), so both were taken back.  Timed against the parent (docs/NOTEBOOK.md, round 16): ..._cx_side_pc<2> 7.3-7.4 us against
// 7.0 in each of six alternated pairs, which is below the three-spreads threshold; the other forms no different.
template <int CPR, int UNR, bool NT>
struct SideRows {
    static constexpr int RPW = 64 / CPR;   // rows per wave step
    const u32x4 *ov;
    const uint32_t *ov_row;
    uint64_t n_ov;
    uint64_t m1a, m1b, m0a, m0b;           // this lane's two words of each mask
    int lane, g;

    __device__ __forceinline__ SideRows(const u32x4 *ov_, const uint32_t *ov_row_, uint64_t n_ov_, const uint64_t *m1, const uint64_t *m0)
        : ov(ov_), ov_row(ov_row_), n_ov(n_ov_)
    {
        lane = threadIdx.x & 63;
        g = lane & (CPR - 1);
        m1a = m1[2 * g]; m1b = m1[2 * g + 1]; m0a = m0[2 * g]; m0b = m0[2 * g + 1];
    }
    __device__ __forceinline__ uint64_t n_steps() const { return (n_ov + RPW - 1) / RPW; }
    __device__ __forceinline__ void load(u32x4 (&x)[UNR], uint64_t s0) const
    {
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const uint64_t r = (s0 + u) * RPW + lane / CPR;
            x[u] = r < n_ov ? (NT ? __builtin_nontemporal_load(&ov[r * CPR + g]) : ov[r * CPR + g]) : (u32x4)(0u);
        }
    }
    __device__ __forceinline__ void evaluate(const u32x4 (&x)[UNR], uint64_t s0, const ScanCuts &K, const ScanSink &S) const
    {
        uint32_t ac[UNR], pend = 0;   // a | c << 16 of the batch's rows; bit u: row u passed the filter and the pre-test
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const uint64_t r = (s0 + u) * RPW + lane / CPR;
            const uint64_t xa = ((uint64_t)x[u].y << 32) | x[u].x, xb = ((uint64_t)x[u].w << 32) | x[u].z;
            uint32_t a = __popcll(xa & m1a) + __popcll(xb & m1b);
            uint32_t c = __popcll(xa & m0a) + __popcll(xb & m0b);
            if (CPR == 2) {
                a += __shfl_xor(a, 1, 64);
                c += __shfl_xor(c, 1, 64);
            }
            // by hand what chi2_candidate(K, a, c, r < n_ov, g == 0) does (see above)
            const int n_w = (int)(a + c);
            const int n_wo = (K.n1 - (int)a) + (K.n0 - (int)c);
            const bool freq_ok = (r < n_ov) && !(n_w < K.min_samples || n_wo < 2 || n_w > K.max_samples);
            const double A = (double)a, B = (double)(K.n1 - (int)a), C = (double)c, D = (double)(K.n0 - (int)c);
            ac[u] = a | (c << 16);
            if (freq_ok && g == 0 && chi2_pretest(A, B, C, D, K.thr)) pend |= 1u << u;
        }
        // the exact decision, one copy of it: almost no row gets here, and UNR copies in line cost the streaming part
        // its registers (122 VGPRs against 64 at UNR = 4).  Ascending u, as the in-line form appended them.
        while (pend) {
            const int u = __builtin_ctz(pend);
            pend &= pend - 1;
            uint32_t v = ac[0];
#pragma unroll
            for (int j = 1; j < UNR; j++) v = u == j ? ac[j] : v;
            const uint64_t r = (s0 + u) * RPW + lane / CPR;
            chi2_evaluate(K, S, ov_row[r], (int)(v & 0xffffu), (int)(v >> 16));
        }
    }
};

template <int CPR>
__global__ __launch_bounds__(SC_THREADS) void chi2_scan_kernel_cx(const CxScanArgs X)
{
    static_assert(SC_THREADS == CX_MAX_SAMPLES, "the class table is filled one sample per thread");
    const ScanArgs &P = X.s;
    __shared__ uint16_t s_cls[CX_MAX_SAMPLES];
    stamp_scan_start(P.sink);
    const int lane = threadIdx.x & 63;
    if (blockIdx.x < X.slot_blocks) {
        {
            const int t = threadIdx.x;
            const uint64_t b = 1ull << (t & 63);
            s_cls[t] = (P.m1_inl[t >> 6] & b) ? 1 : (P.m0_inl[t >> 6] & b) ? 0x100 : 0;
        }
        __syncthreads();
        const uint64_t n_pairs = (P.M + 1) / 2;   // the buffer holds whole pairs; an odd last row's partner is not a row
        const uint64_t wave = (uint64_t)blockIdx.x * (SC_THREADS / 64) + (threadIdx.x >> 6);
        const uint64_t stride = (uint64_t)X.slot_blocks * (SC_THREADS / 64) * 64 * CX_UNROLL;
        for (uint64_t p0 = wave * 64 * CX_UNROLL; p0 < n_pairs; p0 += stride) {
            u32x4 x[CX_UNROLL];
#pragma unroll
            for (int u = 0; u < CX_UNROLL; u++) {
                const uint64_t pi = p0 + u * 64 + lane;
                x[u] = pi < n_pairs ? (PSK_CX_NT ? __builtin_nontemporal_load(&X.slots[pi]) : X.slots[pi]) : (u32x4)(0u);
            }
#pragma unroll
            for (int u = 0; u < CX_UNROLL; u++)
#pragma unroll
                for (int sub = 0; sub < 2; sub++) {
                    const uint64_t row = 2 * (p0 + u * 64 + lane) + sub;
                    const uint32_t lo = sub ? x[u].z : x[u].x, hi = sub ? x[u].w : x[u].y;
                    const uint32_t h = lo & 0xffu;
                    if (row >= P.M || (h & CX_HDR_OVF) || !((X.class_mask >> (h & 15u)) & 1u)) continue;
                    const uint32_t e = h & 7u;
                    uint32_t sum = 0;
                    if (e > 0) sum += s_cls[(lo >> 8) & 0xffu];
                    if (e > 1) sum += s_cls[(lo >> 16) & 0xffu];
                    if (e > 2) sum += s_cls[lo >> 24];
                    if (e > 3) sum += s_cls[hi & 0xffu];
                    if (e > 4) sum += s_cls[(hi >> 8) & 0xffu];
                    if (e > 5) sum += s_cls[(hi >> 16) & 0xffu];
                    if (e > 6) sum += s_cls[hi >> 24];
                    int a = (int)(sum & 0xffu), c = (int)(sum >> 8);   // (a', c'): at most e <= 7 each
                    const bool absent = (h & CX_HDR_BASE) != 0;
                    if (!((X.corner[absent ? 1 : 0] >> (a * 8 + c)) & 1ull)) continue;
                    if (absent) { a = P.cut.n1 - a; c = P.cut.n0 - c; }
                    chi2_evaluate(P.cut, P.sink, row, a, c);
                }
        }
    } else if (blockIdx.x - X.slot_blocks < X.ov_blocks) {
        const SideRows<CPR, CX_UNROLL, PSK_CX_NT != 0> R(X.ov, X.ov_row, X.n_ov, P.m1_inl, P.m0_inl);
        const uint64_t wave = (uint64_t)(blockIdx.x - X.slot_blocks) * (SC_THREADS / 64) + (threadIdx.x >> 6);
        const uint64_t total_waves = (uint64_t)X.ov_blocks * (SC_THREADS / 64);
        const uint64_t n_steps = R.n_steps();
        for (uint64_t s0 = wave * CX_UNROLL; s0 < n_steps; s0 += total_waves * CX_UNROLL) {
            u32x4 x[CX_UNROLL];
            R.load(x, s0);
            R.evaluate(x, s0, P.cut, P.sink);
        }
    }
    publish_segment(P.sink);
}

// ---- the side matrix alone: what every scan with no feasible class launches (the Bonferroni scans of a real run) ------
// The mixed kernel above gives the side matrix one batch per wave; its registers are the slot branch's and its 864 bytes
// of arguments every form's.  Here the arguments are what the rows need, there is no LDS, and the grid is what stays
// resident (cx_side_shape): every wave walks its batches grid-stride and has the next batch's loads in flight while it
// evaluates the current one (two register sets, swapped by unrolling the loop twice).
template <int CPR>
__global__ __launch_bounds__(SC_THREADS) void chi2_scan_kernel_cx_side(const CxSideArgs X)
{
    stamp_scan_start(X.sink);
    const SideRows<CPR, CX_SIDE_UNROLL, PSK_CX_SIDE_NT != 0> R(X.ov, X.ov_row, X.n_ov, X.m1, X.m0);
    const uint64_t stride = (uint64_t)gridDim.x * CX_WAVES * CX_SIDE_UNROLL;
    const uint64_t n_steps = R.n_steps();
    uint64_t s0 = ((uint64_t)blockIdx.x * CX_WAVES + (threadIdx.x >> 6)) * CX_SIDE_UNROLL;
    u32x4 xa[CX_SIDE_UNROLL], xb[CX_SIDE_UNROLL];
    if (s0 < n_steps) R.load(xa, s0);
    while (s0 < n_steps) {
        if (s0 + stride < n_steps) R.load(xb, s0 + stride);
        R.evaluate(xa, s0, X.cut, X.sink);
        s0 += stride;
        if (!(s0 < n_steps)) break;
        if (s0 + stride < n_steps) R.load(xa, s0 + stride);
        R.evaluate(xb, s0, X.cut, X.sink);
        s0 += stride;
    }
#ifdef PSK_CX_SIDE_TWO_ATOMICS   // A/B builds: the other kernels' publish (r13: 13.4-13.6 us against 13.1-13.2)
    publish_segment(X.sink);
#else
    publish_segment_once(X.sink);
#endif
}

// ---- the side matrix through its popcounts: the rows a scan's parameters cannot rule out --------------------------
// A row's table (a, c) has a + c within n_na of its popcount, and for a fixed a + c the pre-test is decided at the two
// ends of a's range (cx_pc_plan), so a popcount none of whose sums passes the filter and the pre-test rules the row out
// before it is read: the encoder's 2-byte popcount (cx_ov_pc) is all the kernel loads of it.  A lane owns a row: lane l
// of a wave loads the popcounts of rows b * 64 U + 64 j + l, j = 0 .. U - 1, back to back (128 contiguous bytes per wave
// instruction, 64 U rows per round), then walks j; a row whose bit of `feas` is set -- a live row -- loads its own CPR
// chunks, counts them against the mask words (scalars from the arguments: no shuffle) and takes SideRows::evaluate's
// path from there: the candidate rule in line, the exact decision as one copy per batch.  A row that is
// not live is left out by that predicate alone.  Batches go to the waves grid-stride with the next batch's popcounts
// in flight, as in chi2_scan_kernel_cx_side.
template <int CPR>
struct PcRows {
    static constexpr int U = CX_PC_UNROLL;
    const u32x4 *ov;
    const uint32_t *ov_row;
    const uint16_t *ov_pc;
    uint64_t n_ov;
    uint64_t f0, f1, f2, f3;               // feas
    uint64_t m1[2 * CPR], m0[2 * CPR];     // the mask words of a row's chunks
    int lane;

    __device__ __forceinline__ PcRows(const CxSidePcArgs &X)
        : ov(X.s.ov), ov_row(X.s.ov_row), ov_pc(X.ov_pc), n_ov(X.s.n_ov), f0(X.feas[0]), f1(X.feas[1]), f2(X.feas[2]), f3(X.feas[3])
    {
        lane = threadIdx.x & 63;
#pragma unroll
        for (int i = 0; i < 2 * CPR; i++) { m1[i] = X.s.m1[i]; m0[i] = X.s.m0[i]; }
    }
    __device__ __forceinline__ uint64_t n_batches() const { return (n_ov + 64 * U - 1) / (64 * U); }
    __device__ __forceinline__ uint64_t row(uint64_t b, int j) const { return (b * U + j) * 64 + lane; }
    __device__ __forceinline__ void load(uint32_t (&pc)[U], uint64_t b) const
    {
#pragma unroll
        for (int j = 0; j < U; j++) {
            const uint64_t r = row(b, j);
            pc[j] = r < n_ov ? (PSK_CX_PC_NT ? __builtin_nontemporal_load(&ov_pc[r]) : ov_pc[r]) : 0u;
        }
    }
    __device__ __forceinline__ void evaluate(const uint32_t (&pc)[U], uint64_t b, const ScanCuts &K, const ScanSink &S) const
    {
        uint32_t ac[U], pend = 0;   // a | c << 16 of the batch's live rows; bit j: row j passed the filter and the pre-test
#pragma unroll
        for (int j = 0; j < U; j++) {
            const uint64_t r = row(b, j);
            const uint32_t w = pc[j] >> 6;
            // the 4-way select as masks: a chain of selects of the four words is turned into a table on the stack
            const uint64_t word = (w == 0 ? f0 : 0ull) | (w == 1 ? f1 : 0ull) | (w == 2 ? f2 : 0ull) | (w == 3 ? f3 : 0ull);
            const bool live = r < n_ov && ((word >> (pc[j] & 63u)) & 1ull);
            uint32_t a = 0, c = 0;
            if (live) {
#pragma unroll
                for (int g = 0; g < CPR; g++) {
                    const u32x4 x = PSK_CX_SIDE_NT ? __builtin_nontemporal_load(&ov[r * CPR + g]) : ov[r * CPR + g];
                    const uint64_t xa = ((uint64_t)x.y << 32) | x.x, xb = ((uint64_t)x.w << 32) | x.z;
                    a += __popcll(xa & m1[2 * g]) + __popcll(xb & m1[2 * g + 1]);
                    c += __popcll(xa & m0[2 * g]) + __popcll(xb & m0[2 * g + 1]);
                }
            }
            // by hand what chi2_candidate(K, a, c, live) does (see SideRows)
            const int n_w = (int)(a + c);
            const int n_wo = (K.n1 - (int)a) + (K.n0 - (int)c);
            const bool freq_ok = live && !(n_w < K.min_samples || n_wo < 2 || n_w > K.max_samples);
            const double A = (double)a, B = (double)(K.n1 - (int)a), C = (double)c, D = (double)(K.n0 - (int)c);
            ac[j] = a | (c << 16);
            if (freq_ok && chi2_pretest(A, B, C, D, K.thr)) pend |= 1u << j;
        }
        while (pend) {   // the exact decision, one copy of it (SideRows::evaluate)
            const int j = __builtin_ctz(pend);
            pend &= pend - 1;
            uint32_t v = ac[0];
#pragma unroll
            for (int i = 1; i < U; i++) v = j == i ? ac[i] : v;
            chi2_evaluate(K, S, ov_row[row(b, j)], (int)(v & 0xffffu), (int)(v >> 16));
        }
    }
};

template <int CPR>
__global__ __launch_bounds__(SC_THREADS) void chi2_scan_kernel_cx_side_pc(const CxSidePcArgs X)
{
    stamp_scan_start(X.s.sink);
    const PcRows<CPR> R(X);
    const uint64_t stride = (uint64_t)gridDim.x * CX_WAVES;
    const uint64_t n_batches = R.n_batches();
    uint64_t b = (uint64_t)blockIdx.x * CX_WAVES + (threadIdx.x >> 6);
    uint32_t pa[CX_PC_UNROLL], pb[CX_PC_UNROLL];
    if (b < n_batches) R.load(pa, b);
    while (b < n_batches) {
        if (b + stride < n_batches) R.load(pb, b + stride);
        R.evaluate(pa, b, X.s.cut, X.s.sink);
        b += stride;
        if (!(b < n_batches)) break;
        if (b + stride < n_batches) R.load(pa, b + stride);
        R.evaluate(pb, b, X.s.cut, X.s.sink);
        b += stride;
    }
    publish_segment_once(X.s.sink);
}

// ---- the feasible rows of the side matrix through the encoder's index --------------------------------------------------
// Which rows have a given popcount is a property of the matrix, so the encoder groups the side-matrix rows by popcount
// once (cx_pc_index, presence_compact.hip) and a scan whose feasible popcounts hold few rows (cx_idx_chosen, chi2_plan.h)
// visits those rows alone: the T rows of at most CX_IDX_RUNS ranges of the index, one per lane, grid-stride.  Lane t
// finds its range against the running sums of run_len, loads j = idx[...], then the row's CPR chunks AND ov_row[j]
// together (the row id does not wait for the decision: every row here is likely to be a candidate), counts against the
// scalar mask words and decides as PcRows does: the candidate rule by hand in the same operations, chi2_keep.  At the
// flagship every such row survives, so the appends are taken per wave: one atomicAdd of the keepers' number, each keeper
// at base + its rank, clamped as reserve_slot clamps (an overflow still reaches the host as a count above seg_cap).
// As many workgroups as the rows need: the segments beyond the grid are published by workgroup 0 before its rows.
// Up to SC_NSEG one-wave workgroups (the flagship: 28), each is its segment's only writer and counts its keepers in a
// register: the append and the publish atomics above are the launches' of more workgroups than segments (r31).
template <int CPR>
__global__ __launch_bounds__(CX_IDX_THREADS) void chi2_scan_kernel_cx_side_idx(const CxSideIdxArgs X)
{
    const ScanCuts &K = X.s.cut;
    const ScanSink &S = X.s.sink;
    stamp_scan_start(S);
    if (blockIdx.x == 0) publish_unowned_segments(S);
    const int lane = threadIdx.x & 63;
    const uint64_t e0 = X.run_len[0], e1 = e0 + X.run_len[1], e2 = e1 + X.run_len[2], T = e2 + X.run_len[3];
    const uint32_t seg = blockIdx.x & (SC_NSEG - 1);
    // A workgroup of one wave in a launch of at most SC_NSEG workgroups is its segment's only writer, so the wave keeps the
    // segment's count itself (r31): no atomic per append, none to publish -- the segment's counter line is never touched
    // and stands at zero for the next scan -- and the one atomic round trip left in its tail is the summary's ticket.
    const bool sole = CX_IDX_THREADS == 64 && gridDim.x <= (uint32_t)SC_NSEG;
    uint32_t n_own = 0;   // wave-uniform
    // (t0 is the workgroup's: whole waves walk the loop, the ballot below sees all 64 lanes)
    for (uint64_t t0 = (uint64_t)blockIdx.x * CX_IDX_THREADS; t0 < T; t0 += (uint64_t)gridDim.x * CX_IDX_THREADS) {
        const uint64_t t = t0 + threadIdx.x;
        const bool live = t < T;
        uint32_t a = 0, c = 0, row = 0;
        if (live) {
            const uint64_t pos = t < e0 ? X.run_begin[0] + t : t < e1 ? X.run_begin[1] + (t - e0) : t < e2 ? X.run_begin[2] + (t - e1) : X.run_begin[3] + (t - e2);
            const uint64_t j = X.idx[pos];
            u32x4 x[CPR];
#pragma unroll
            for (int g = 0; g < CPR; g++) x[g] = PSK_CX_SIDE_NT ? __builtin_nontemporal_load(&X.s.ov[j * CPR + g]) : X.s.ov[j * CPR + g];
            row = X.s.ov_row[j];
#pragma unroll
            for (int g = 0; g < CPR; g++) {
                const uint64_t xa = ((uint64_t)x[g].y << 32) | x[g].x, xb = ((uint64_t)x[g].w << 32) | x[g].z;
                a += __popcll(xa & X.s.m1[2 * g]) + __popcll(xb & X.s.m1[2 * g + 1]);
                c += __popcll(xa & X.s.m0[2 * g]) + __popcll(xb & X.s.m0[2 * g + 1]);
            }
        }
        // by hand what chi2_candidate(K, a, c, live) does (see SideRows)
        const int n_w = (int)(a + c);
        const int n_wo = (K.n1 - (int)a) + (K.n0 - (int)c);
        const bool freq_ok = live && !(n_w < K.min_samples || n_wo < 2 || n_w > K.max_samples);
        const double A = (double)a, B = (double)(K.n1 - (int)a), C = (double)c, D = (double)(K.n0 - (int)c);
        double stat = 0.0, p = 1.0;
        bool keep = false;
        if (freq_ok && chi2_pretest(A, B, C, D, K.thr)) keep = chi2_keep(K, A, B, C, D, stat, p);
        const uint64_t keepers = __ballot(keep);
        if (keepers) {   // wave-uniform
            uint32_t base = n_own;
            if (sole) n_own += (uint32_t)__popcll(keepers);
            else {
                if (lane == 0) base = atomicAdd(&S.counter[seg * SC_CNT_STRIDE], (uint32_t)__popcll(keepers));
                base = __builtin_amdgcn_readfirstlane(base);
            }
            if (keep) {
                const uint32_t idx = base + (uint32_t)__popcll(keepers & ((1ull << lane) - 1ull));
                chi2_store(S, (uint64_t)seg * S.seg_cap + (idx < S.seg_cap ? idx : S.seg_cap - 1), row, stat, p, n_w);
            }
        }
    }
    if (sole) {   // (the wave's own stores need no barrier before its own publish)
        if (threadIdx.x == 0) {
            S.final_counts[seg] = n_own;
            stamp_segment(S, seg, n_own);
        }
    } else publish_segment_once(S);
}

// Second pass of the weighted chi2 scan: one workgroup per result segment, one candidate per lane.  The 2 x 2 table is
// summed again exactly as the reference does it (modeling.py:809-823: every sample in order adds its weight to ONE of
// the four cells; here the other three get + 0.0, and a weight times 1.0 or 0.0 is exact, so one fma per cell IS that
// addition), so the statistic, round(chi2, 2) and "%.2E" of the
// p-value are the reference's to the last bit; then the keep rule of modeling.py:795 and the compaction of the segment
// in place.  (Doing this inside the scan kernel, per 64 queued rows with at least one candidate, cost 2.3 ms instead of
// 0.6 ms for 16 M x 1024: the sample-order sums are a dependent chain of 1024 f64 adds whatever the number of live lanes.)
__global__ __launch_bounds__(SC_FIN_THREADS) void chi2w_finalize_kernel(const ScanArgs P)
{
    __shared__ uint32_t scan_lds[SC_FIN_THREADS / 64];
    __shared__ uint32_t s_out;
    // {weight if phenotype 1, weight if phenotype 0} of the samples of the current block: every lane reads the SAME
    // entry at the same time (one broadcast ds_read_b128).  As scalar loads from global memory the entries cost
    // ~330 cycles per sample (0.14 ms for 160 k candidates of 1024 samples); from LDS the pass is its 4 + 3 VALU
    // operations per sample.
    __shared__ double2 s_tab[SC_FIN_BLK * 128];
    const uint32_t seg = blockIdx.x;
    const uint32_t c = P.sink.counter[seg * SC_CNT_STRIDE];
    const uint64_t base = (uint64_t)seg * P.sink.seg_cap;
    if (threadIdx.x == 0) s_out = 0;
    __syncthreads();
    for (uint32_t s0 = 0; s0 < c; s0 += SC_FIN_THREADS) {
        const uint32_t i = s0 + threadIdx.x;
        const bool valid = i < c;
        const uint64_t row = valid ? P.sink.res_row[base + i] : 0;
        const int32_t nw = valid ? P.sink.res_nw[base + i] : 0;
        const bool wave_any = __any(valid);
        const u32x4 *rp = P.half ? sc_row_ptr<true>(P, row) : sc_row_ptr<false>(P, row);
        // the four cells, sample by sample
        double ca = 0.0, cb = 0.0, cc = 0.0, cd = 0.0;
        for (int c0 = 0; c0 < P.cpr; c0 += SC_FIN_BLK) {
            const int nc = P.cpr - c0 < SC_FIN_BLK ? P.cpr - c0 : SC_FIN_BLK;
            __syncthreads();   // the previous block has been consumed
            for (int e = threadIdx.x; e < nc * 128; e += SC_FIN_THREADS)
                s_tab[e] = reinterpret_cast<const double2 *>(P.tab)[(size_t)c0 * 128 + e];
            __syncthreads();
            if (!wave_any) continue;
            for (int ch = 0; ch < nc; ch++) {
                const u32x4 y = P.half ? sc_ld_chunk<true>(rp, 0) : rp[c0 + ch];   // (an 8-byte row: samples 64 ... 127 have zero weights)
                const uint32_t w4[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                for (int h = 0; h < 4; h++) {
#pragma unroll 8
                    for (int sb = 0; sb < 32; sb++) {
                        const uint32_t fh = (uint32_t)(((int32_t)(w4[h] << (31 - sb))) >> 31) & 0x3FF00000u;
                        const double f = __hiloint2double((int)fh, 0), g = __hiloint2double((int)(fh ^ 0x3FF00000u), 0);
                        const double2 t = s_tab[ch * 128 + h * 32 + sb];
                        ca = fma(f, t.x, ca);
                        cb = fma(g, t.x, cb);
                        cc = fma(f, t.y, cc);
                        cd = fma(g, t.y, cd);
                    }
                }
            }
        }
        double stat = 0.0, p = 1.0;
        bool keep = false;
        if (wave_any) keep = chi2_keep(P.cut, ca, cb, cc, cd, stat, p, valid);
        uint32_t tot;
        const uint32_t pos = psk_block_excl_scan_u32<SC_FIN_THREADS>(keep ? 1u : 0u, &tot, scan_lds);  // barriers inside
        const uint32_t out = s_out;
        if (keep) chi2_store(P.sink, base + out + pos, row, stat, p, nw);  // <= base + i: compaction only moves entries down
        __syncthreads();
        if (threadIdx.x == 0) s_out = out + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        P.sink.counter[seg * SC_CNT_STRIDE] = 0;  // re-armed for the next scan
        P.sink.final_counts[seg] = s_out;
        stamp_count(P.sink, seg, s_out);
    }
}

template <int MODE, bool LUT = false, bool F32 = false>
void launch_chi2_form(int G, dim3 grid, size_t lds, hipStream_t st, TimedBy ev, const ScanArgs &a)
{
    dispatch_G<LUT ? 16 : 64>(G, [&](auto g) {
        launch_timed(chi2_scan_kernel<decltype(g)::value, MODE, LUT, F32>, grid, LUT ? SC_LUT_THREADS : SC_THREADS, lds, st, ev, a);
    });
}

// (the weighted form is two kernels: the scan's time runs from the start of the first to the end of the second)
void launch_chi2(int mode, int G, dim3 grid, hipStream_t st, TimedBy ev, const ScanArgs &a)
{
    if (mode == 1) {
        if (a.lut6) launch_chi2_form<1, true, true>(G, grid, lut6_bytes(a.cpr, 2), st, ev.first(), a);
        else if (a.lut) launch_chi2_form<1, true>(G, grid, lut_bytes(a.c_lut, 2), st, ev.first(), a);
        else launch_chi2_form<1>(G, grid, 0, st, ev.first(), a);
        launch_timed(chi2w_finalize_kernel, dim3(SC_NSEG), SC_FIN_THREADS, 0, st, ev.last(), a);
    }
    else if (mode == 2) launch_chi2_form<2>(G, grid, 0, st, ev, a);
    else launch_chi2_form<0>(G, grid, 0, st, ev, a);
}

}  // namespace

void launch_chi2_any(psk_ctx *ctx, const Chi2Launch &L, TimedBy ev)
{
    const hipStream_t st = ctx->stream;
    switch (L.form) {
    case Chi2Form::CxSideIdx:
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx_side_idx<1>, L.grid, CX_IDX_THREADS, 0, st, ev, L.sidx);
        else launch_timed(chi2_scan_kernel_cx_side_idx<2>, L.grid, CX_IDX_THREADS, 0, st, ev, L.sidx);
        break;
    case Chi2Form::CxSidePc:
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx_side_pc<1>, L.grid, SC_THREADS, 0, st, ev, L.side);
        else launch_timed(chi2_scan_kernel_cx_side_pc<2>, L.grid, SC_THREADS, 0, st, ev, L.side);
        break;
    case Chi2Form::CxSide:
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx_side<1>, L.grid, SC_THREADS, 0, st, ev, L.side.s);
        else launch_timed(chi2_scan_kernel_cx_side<2>, L.grid, SC_THREADS, 0, st, ev, L.side.s);
        break;
    case Chi2Form::CxMixed:
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx<1>, L.grid, SC_THREADS, 0, st, ev, L.x);
        else launch_timed(chi2_scan_kernel_cx<2>, L.grid, SC_THREADS, 0, st, ev, L.x);
        break;
    case Chi2Form::Dense:
        launch_chi2(L.mode, group_lanes(L.x.s), L.grid, st, ev, L.x.s);
        break;
    }
}
