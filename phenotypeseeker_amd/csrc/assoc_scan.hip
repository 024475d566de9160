// a4-a7: per-k-mer association scans over the bit-packed presence matrix -- the chi2 scans.
//
// chi2_scan_kernel   replaces phenotypes.get_kmers_tested / conduct_chi_squared_test and helpers
//                    (modeling.py:677-714, :759-858)
// ttest_scan_kernel  (ttest_scan.hip) replaces conduct_t_test / get_samples_distribution_for_ttest (:716-757)
// chi2_scan_kernel_cx  the unweighted chi2 scan over the exception-coded copy of the matrix (presence_compact.hip), when
//                      there is one: same survivors, a third of the bytes at config 2
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
// runs on rows that a division-free test T*(ad-bc)^2 >= thr*R1*R0*K1*K0*(1-1e-9) cannot rule out.
#include "scan_common.h"
#include "cx_side_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

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

// the division-free pre-test of a unit-weight 2 x 2 table: chi2 = T (AD - BC)^2 / (R1 R0 K1 K0) cannot be ruled out
// against thr.  Host and device evaluate it in the same IEEE double operations (-ffp-contract=off): the host's corner
// table of the exception-coded scan (cx_plan) decides bit for bit what the dense kernel decides.
__host__ __device__ __forceinline__ bool chi2_pretest(double A, double B, double C, double D, double thr)
{
    const double R1 = A + B, R0 = C + D, K1 = A + C, K0 = B + D, T = R1 + R0;
    const double det = A * D - B * C;
    const double lhs = T * det * det, rhs = thr * R1 * R0 * K1 * K0;
    return !(lhs < rhs * (1.0 - 1e-9));  // NaN compares false -> a candidate
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

// chi2_scan_kernel MODE 0 from the two class counts of a row
__device__ __forceinline__ void chi2_evaluate(const ScanCuts &K, const ScanSink &S, uint64_t row, int a, int c)
{
    double stat, p;
    if (chi2_keep(K, (double)a, (double)(K.n1 - a), (double)c, (double)(K.n0 - c), stat, p)) chi2_store(S, reserve_slot(S), row, stat, p, a + c);
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
        const int n_w = (int)(a + c);
        const int n_wo = (P.cut.n1 - (int)a) + (P.cut.n0 - (int)c);
        const bool freq_ok = (row < P.M) && !(n_w < P.cut.min_samples || n_wo < 2 || n_w > P.cut.max_samples);
        if (WEIGHTED) {
            Q.n = queue_rows(freq_ok && lead, row, make_int2(n_w, 0), Q.row, Q.val, Q.n, lane);
            return;
        }
        const double A = (double)a, B = (double)(P.cut.n1 - (int)a), C = (double)c, D = (double)(P.cut.n0 - (int)c);
        const bool cand = freq_ok && lead && chi2_pretest(A, B, C, D, P.cut.thr);
        if (MODE == 2) {
            Q.n = queue_rows(cand, row, make_int2((int)a, (int)c), Q.row, Q.val, Q.n, lane);
            return;
        }
        if (cand) chi2_decide(P, row, A, B, C, D, n_w);
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
// filter and the division-free pre-test -- is one bit of the two corner words the host filled for this scan (cx_plan: the
// same double operations as chi2_pretest); candidates take chi2_scan_kernel's MODE 0 path (chi2_exact, exp, keep rule), so
// stat and p are the dense kernel's bits.  A header class (e, base) none of whose reachable corner points is a candidate
// is dropped on the header byte (X.class_mask); when NO class is feasible -- every Bonferroni cut-off of a real run: a row
// of at most 7 exceptions cannot reach the statistic -- the host launches no slot workgroup and the slots are not read.
// The rows with more than CX_MAX_E exceptions are a side matrix of dense rows that the last workgroups of the SAME launch
// scan as chi2_scan_kernel's MODE 0 does (CPR 16-byte chunks per row, one lane each; frequency filter and chi2_pretest
// in line), reporting their original row ids: a second launch would add a kernel boundary to every step.
#ifndef PSK_CX_UNROLL
#define PSK_CX_UNROLL 4
#endif
#ifndef PSK_CX_NT
#define PSK_CX_NT 0   // plain loads: 57.4 us against 60.7 us with the nontemporal hint at config 2
#endif
#ifndef PSK_CX_SIDE_NT
#define PSK_CX_SIDE_NT 1   // nontemporal hint on the side matrix: lower in five of six pairs of the r13 table (docs/NOTEBOOK.md), also re-read launch after launch
#endif
#ifndef PSK_CX_SIDE_GRID_MULT
#define PSK_CX_SIDE_GRID_MULT 8   // workgroups per CU of chi2_scan_kernel_cx_side when PSK_GRID_MULT is unset (r13 table: 8 before 4 and the one-batch grid)
#endif
constexpr int CX_UNROLL = PSK_CX_UNROLL;   // 16-byte loads in flight per lane
static_assert(CX_SIDE_WAVES * 64 == SC_THREADS && CX_SIDE_NSEG == SC_NSEG, "cx_side_plan.h restates the launch constants");

// The rows of the side matrix, once: UNR wave steps of 64 / CPR rows from step s0 on, one lane per 16-byte chunk.
// load() issues the batch's loads; evaluate() is chi2_scan_kernel MODE 0's on_row on what came back -- popcounts against
// the lane's mask words, the sum over the row's CPR lanes, frequency filter and chi2_pretest in line, then the exact
// decision -- and reports a survivor under its original row id.  Both are called by whole waves (the CPR = 2 shuffle).
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
            // chi2_scan_kernel MODE 0's on_row
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

struct CxScanArgs {
    ScanArgs s;                  // the scan: unit weights, masks inline
    const u32x4 *slots;          // two slots per 16 bytes
    const u32x4 *ov;             // overflow rows, dense, cpr chunks each, ascending
    const uint32_t *ov_row;      // ... their row ids
    uint64_t n_ov;
    uint32_t slot_blocks;        // workgroups [0, slot_blocks) stream the slots (none when no class is feasible),
    uint32_t ov_blocks;          // the next ov_blocks the overflow rows; any beyond only publish their segment
    uint32_t class_mask;         // bit (header & 15): some reachable table of that e and base is a candidate (cx_plan)
    uint64_t corner[2];          // [base] bit a' * 8 + c': the table (a', c') / (n1 - a', n0 - c') is a candidate
};

template <int CPR>
__global__ __launch_bounds__(SC_THREADS) void chi2_scan_kernel_cx(const CxScanArgs X)
{
    static_assert(SC_THREADS == CX_MAX_SAMPLES, "the class table is filled one sample per thread");
    const ScanArgs &P = X.s;
    __shared__ uint16_t s_cls[CX_MAX_SAMPLES];
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
struct CxSideArgs {
    const u32x4 *ov;
    const uint32_t *ov_row;
    uint64_t n_ov;
    uint64_t m1[4], m0[4];       // the mask words of the row's (at most two) chunks
    ScanCuts cut;
    ScanSink sink;
};
static_assert(sizeof(CxSideArgs) <= 256, "chi2_scan_kernel_cx_side's arguments are meant to stay small");

template <int CPR>
__global__ __launch_bounds__(SC_THREADS) void chi2_scan_kernel_cx_side(const CxSideArgs X)
{
    const SideRows<CPR, CX_SIDE_UNROLL, PSK_CX_SIDE_NT != 0> R(X.ov, X.ov_row, X.n_ov, X.m1, X.m0);
    const uint64_t stride = (uint64_t)gridDim.x * CX_SIDE_WAVES * CX_SIDE_UNROLL;
    const uint64_t n_steps = R.n_steps();
    uint64_t s0 = ((uint64_t)blockIdx.x * CX_SIDE_WAVES + (threadIdx.x >> 6)) * CX_SIDE_UNROLL;
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
// path from there: frequency filter and chi2_pretest in line, the exact decision as one copy per batch.  A row that is
// not live is left out by that predicate alone.  Batches go to the waves grid-stride with the next batch's popcounts
// in flight, as in chi2_scan_kernel_cx_side.
#ifndef PSK_CX_PC_NT
#define PSK_CX_PC_NT 0   // nontemporal hint on the popcount loads
#endif
#ifndef PSK_CX_PC_GRID_MULT
#define PSK_CX_PC_GRID_MULT 8   // workgroups per CU when PSK_GRID_MULT is unset
#endif
struct CxSidePcArgs {
    CxSideArgs s;
    const uint16_t *ov_pc;       // popcount of every side-matrix row over the valid samples
    uint64_t feas[4];            // bit pc: a row of that popcount can be a candidate
};
static_assert(sizeof(CxSidePcArgs) <= 256, "chi2_scan_kernel_cx_side_pc's arguments are meant to stay small");

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
            // chi2_scan_kernel MODE 0's on_row
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
    const PcRows<CPR> R(X);
    const uint64_t stride = (uint64_t)gridDim.x * CX_SIDE_WAVES;
    const uint64_t n_batches = R.n_batches();
    uint64_t b = (uint64_t)blockIdx.x * CX_SIDE_WAVES + (threadIdx.x >> 6);
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
        P.sink.host_counts[seg] = s_out;
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

// Kernel form of a chi2 scan.  Unit weights: MODE 2 (queued candidates) when many rows are expected to pass the
// pre-test -- the last chi2 scan of this matrix kept more than 0.1 % of the rows, or, with no history, the keep rule
// itself lets that many through under the null hypothesis (p < cut holds for a fraction `cut` of unassociated rows).
// PSK_CHI2_MODE=0|2 forces one (A/B runs).
int pick_chi2_mode(psk_ctx *ctx, bool weighted, double pcut, double pcut_bonf, int omit_B, int *mode)
{
    double expect = pcut_bonf;
    if (omit_B && pcut > expect) expect = pcut;
    *mode = weighted ? 1 : ctx->dense_hint >= 0 ? (ctx->dense_hint ? 2 : 0) : expect > 1e-3 ? 2 : 0;
    return weighted ? PSK_OK : env_choice(ctx, "PSK_CHI2_MODE", {0, 2}, mode);   // read per scan: tests cross the two forms in one process
}

// ---- exception-coded path: the per-scan plan and the launch shape ----
// What a scan's parameters leave of the slot rows.  corner[base] bit a' * 8 + c' (a', c' <= 7): the table of a slot row
// with a' case and c' control exceptions -- (a', c') when the exceptions are the present samples (base 0), (n1 - a',
// n0 - c') when they are the absent ones (base 1) -- passes chi2_scan_kernel's frequency filter and chi2_pretest (the same
// double operations); 0 where a' > n1 or c' > n0: no row has such a table.  class_mask bit (e | base << 3): a row of e
// exceptions can have a table whose bit is set.  Its a' + c' is e less its exceptions among the NA samples, of which
// there are n_samples - n1 - n0.  (n1 = 0, n0 = 0: the pre-test lets every NaN table through, the filter alone decides.)
void cx_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint32_t *class_mask, uint64_t corner[2])
{
    corner[0] = corner[1] = 0;
    for (int base = 0; base < 2; base++)
        for (int ap = 0; ap <= CX_MAX_E && ap <= n1; ap++)
            for (int cp = 0; cp <= CX_MAX_E && cp <= n0; cp++) {
                const int ai = base ? n1 - ap : ap, ci = base ? n0 - cp : cp;
                const int n_w = ai + ci, n_wo = (n1 - ai) + (n0 - ci);
                const bool freq_ok = !(n_w < min_samples || n_wo < 2 || n_w > max_samples);
                const double A = (double)ai, B = (double)(n1 - ai), C = (double)ci, D = (double)(n0 - ci);
                if (freq_ok && chi2_pretest(A, B, C, D, thr)) corner[base] |= 1ull << (ap * 8 + cp);
            }
    const int n_na = n_samples - n1 - n0;
    *class_mask = 0;
    for (int h = 0; h < 16; h++) {
        const int e = h & 7, base = h >> 3;
        bool ok = false;
        for (int ap = 0; ap <= e && !ok; ap++)
            for (int cp = 0; ap + cp <= e && !ok; cp++)
                ok = ap + cp >= e - n_na && ((corner[base] >> (ap * 8 + cp)) & 1ull);
        if (ok) *class_mask |= 1u << h;
    }
}

// What a scan's parameters leave of the side matrix, by popcount.  Bit pc of feas (pc <= 255: a side-matrix row has
// CX_MAX_E < pc < n_samples - CX_MAX_E) is set exactly when a row of that popcount over the valid samples can have a
// candidate table: its s = a + c is pc less its present NA samples, s in [max(0, pc - n_na), min(pc, n1 + n0)]; the
// frequency filter depends on s alone; and with s fixed det = (n1 + n0) a - n1 s, so chi2_pretest's left side is convex
// in a while its right side does not depend on a -- some table of that s passes exactly when one at a = max(0, s - n0)
// or a = min(s, n1) does.  (Everything in the left side is an integer below 2^53: exact, so "convex" holds in the
// doubles.)  Two pre-tests per s, n1 + n0 + 1 values of s.
void cx_pc_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint64_t feas[4])
{
    const int T = n1 + n0, n_na = n_samples - T;
    std::vector<int> ok_upto(T + 2, 0);   // ok_upto[s + 1]: sums <= s that pass
    for (int s = 0; s <= T; s++) {
        const bool freq_ok = !(s < min_samples || T - s < 2 || s > max_samples);
        bool ok = false;
        if (freq_ok) {
            const int ends[2] = {std::max(0, s - n0), std::min(s, n1)};
            for (int e = 0; e < 2 && !ok; e++) {
                const int a = ends[e], c = s - a;
                ok = chi2_pretest((double)a, (double)(n1 - a), (double)c, (double)(n0 - c), thr);
            }
        }
        ok_upto[s + 1] = ok_upto[s] + (ok ? 1 : 0);
    }
    feas[0] = feas[1] = feas[2] = feas[3] = 0;
    for (int pc = 0; pc < 256; pc++) {
        const int lo = std::max(0, pc - n_na), hi = std::min(pc, T);
        if (lo <= hi && ok_upto[hi + 1] - ok_upto[lo] > 0) feas[pc >> 6] |= 1ull << (pc & 63);
    }
}

// Workgroups of the two parts in proportion to their bytes, under scan_grid's cap; x.slot_blocks = the first part's,
// x.ov_blocks the second's.  With no feasible class (x.class_mask == 0) the slots get none and the side matrix the whole
// cap.  At least SC_NSEG workgroups: every result segment needs one to publish its count and re-arm its counter.
dim3 cx_grid(const psk_ctx *ctx, CxScanArgs &x, int cpr)
{
    const uint64_t wpb = SC_THREADS / 64;
    const uint64_t n_pairs = (x.s.M + 1) / 2, ov_rpw = 64 / cpr;
    uint64_t bs = x.class_mask ? ((n_pairs + 64 * CX_UNROLL - 1) / (64 * CX_UNROLL) + wpb - 1) / wpb : 0;
    uint64_t bo = (((x.n_ov + ov_rpw - 1) / ov_rpw + CX_UNROLL - 1) / CX_UNROLL + wpb - 1) / wpb;
    const uint64_t cap = scan_grid_cap(ctx);
    if (!x.class_mask) bo = std::min(bo, cap);
    else if (bs + bo > cap) {
        const double slot_bytes = 16.0 * n_pairs, ov_bytes = 16.0 * cpr * x.n_ov;
        const uint64_t s = (uint64_t)(cap * slot_bytes / (slot_bytes + ov_bytes) + 0.5);
        bs = std::min(bs, std::max<uint64_t>(s, 1));
        bo = std::min(bo, cap - bs);
        if (x.n_ov && bo == 0) { bo = 1; bs = std::max<uint64_t>(bs - 1, 1); }
    }
    uint64_t total = bs + bo;
    if (total < SC_NSEG) {
        if (x.class_mask) bs = SC_NSEG - bo;   // (more slot workgroups than slot work: they find p0 >= n_pairs)
        total = SC_NSEG;
    }
    x.slot_blocks = (uint32_t)bs;
    x.ov_blocks = (uint32_t)bo;
    return dim3((unsigned)total);
}

// most workgroups of chi2_scan_kernel_cx_side: PSK_GRID_MULT per CU when set, else the kernel's own multiple
uint64_t cx_side_grid_cap(const psk_ctx *ctx) { return (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : PSK_CX_SIDE_GRID_MULT); }
// ... and of chi2_scan_kernel_cx_side_pc
uint64_t cx_pc_grid_cap(const psk_ctx *ctx) { return (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : PSK_CX_PC_GRID_MULT); }

// the most rows one workgroup of chi2_scan_kernel_cx visits
uint64_t cx_rows_per_block(const CxScanArgs &x, int cpr)
{
    const uint64_t wpb = SC_THREADS / 64;
    const uint64_t n_pairs = (x.s.M + 1) / 2, ov_rpw = 64 / cpr;
    const uint64_t ws = (uint64_t)x.slot_blocks * wpb, wo = (uint64_t)x.ov_blocks * wpb;
    const uint64_t cs = (n_pairs + 64 - 1) / 64, co = (x.n_ov + ov_rpw - 1) / ov_rpw;   // wave steps
    const uint64_t rs = ws ? (cs + ws * CX_UNROLL - 1) / (ws * CX_UNROLL) * wpb * CX_UNROLL * 128 : 0;
    const uint64_t ro = wo ? (co + wo * CX_UNROLL - 1) / (wo * CX_UNROLL) * wpb * CX_UNROLL * ov_rpw : 0;
    return std::max(rs, ro);
}

// One chi2 scan as the host launches it: the dense kernels' arguments, and the exception-coded path when it runs
struct Chi2Launch {
    CxScanArgs x;      // x.s: every form's arguments; the rest: chi2_scan_kernel_cx's
    CxSidePcArgs side;   // chi2_scan_kernel_cx_side's (side.s) when the plan says so (side_kernel); all of it: ..._side_pc's (filtered)
    bool compact = false, side_kernel = false, filtered = false;
    int mode = 0;      // of the dense kernels (pick_chi2_mode)
    int cpr = 0;
    dim3 grid;
};

void launch_chi2_any(psk_ctx *ctx, const Chi2Launch &L, TimedBy ev)
{
    const ScanArgs &a = L.x.s;
    if (L.compact && L.side_kernel && L.filtered) {
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx_side_pc<1>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.side);
        else launch_timed(chi2_scan_kernel_cx_side_pc<2>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.side);
        return;
    }
    if (L.compact && L.side_kernel) {
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx_side<1>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.side.s);
        else launch_timed(chi2_scan_kernel_cx_side<2>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.side.s);
        return;
    }
    if (L.compact) {
        if (L.cpr == 1) launch_timed(chi2_scan_kernel_cx<1>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.x);
        else launch_timed(chi2_scan_kernel_cx<2>, L.grid, SC_THREADS, 0, ctx->stream, ev, L.x);
        return;
    }
    launch_chi2(L.mode, group_lanes(a), L.grid, ctx->stream, ev, a);
}

int run_chi2(psk_ctx *ctx, const Chi2Launch &L, int reps, double *ms_total, double *ms_each = nullptr)
{
    *ms_total = 0;
    for (int r = 0; r < reps; r++) {
        launch_chi2_any(ctx, L, {ctx->ev0, ctx->ev1});
        PSK_HIP(ctx, hipGetLastError());
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the kernel has written the counts to pinned memory
        float ms = 0;
        PSK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        *ms_total += ms;
        if (ms_each) ms_each[r] = ms;
    }
    return PSK_OK;
}

}  // namespace

// The arguments of the last chi2 scan (ctx->last) for result set `set`.  Unit weights on a matrix with an exception-coded
// copy run chi2_scan_kernel_cx over it, unless PSK_SCAN_DENSE=1 (read per call: A/B runs and tests in one build).
// build_tables: a new scan, whose weight table has just been uploaded (a repeated scan finds its table in place).
static int fill_chi2_args(psk_ctx *ctx, Chi2Launch &CL, int set, bool build_tables)
{
    const ScanParams &L = ctx->last;
    CL.x.s = ScanArgs();
    ScanArgs &a = CL.x.s;
    a.bits = reinterpret_cast<const u32x4 *>(ctx->bits.p);
    a.M = ctx->n_kmers;
    const int mw = mask_words(ctx);
    a.cpr = mw / 2;
    a.half = ctx->wpr == 1;
    a.m1 = ctx->mask1.as<uint64_t>();
    a.m0 = a.m1 + mw;
    a.tab = reinterpret_cast<const double *>(a.m1 + 2 * (size_t)mw);  // [sample][w if pheno 1 | w if pheno 0]
    a.inline_masks = L.inline_masks;
    if (L.inline_masks) { memcpy(a.m1_inl, L.m1, sizeof(a.m1_inl)); memcpy(a.m0_inl, L.m0, sizeof(a.m0_inl)); }
    a.cut.min_samples = L.min_samples;
    a.cut.max_samples = L.max_samples;
    a.cut.pcut = L.pvalue_cutoff;
    a.cut.pcut_bonf = L.pvalue_cutoff / (double)L.n_kmers_global;
    a.cut.omit_B = L.omit_B;
    double pmax = a.cut.pcut_bonf;
    if (L.omit_B && a.cut.pcut > pmax) pmax = a.cut.pcut;
    if (pmax >= 1.0) a.cut.thr = 0.0;
    else if (pmax <= 0.0) a.cut.thr = INFINITY;
    else a.cut.thr = -2.0 * log(pmax);
    a.W1 = L.W1; a.W0 = L.W0;
    a.cut.n1 = L.n1; a.cut.n0 = L.n0;
    ScanShape sh;   // weighted: class-weight sums from a table in LDS (e0 = class 1, e1 = class 0)
    PSK_TRY(setup_table_scan(ctx, a, L.weighted ? a.tab : nullptr, 2, L.W1, L.W0, 0.0, build_tables, &sh));
    CL.compact = ctx->cx_valid && !L.weighted && L.inline_masks && !env_flag("PSK_SCAN_DENSE");
    ctx->cx_last_plan = false;
    if (CL.compact) {
        CxScanArgs &x = CL.x;
        CL.cpr = a.cpr;
        x.slots = ctx->cx_slots.as<u32x4>();
        x.ov = ctx->cx_ov.as<u32x4>();
        x.ov_row = ctx->cx_ov_row.as<uint32_t>();
        x.n_ov = ctx->cx_n_ov;
        int side_on = 1;   // read per scan: A/B runs and tests in one build
        PSK_TRY(env_choice(ctx, "PSK_CX_SIDE_KERNEL", {0, 1}, &side_on));
        int pc_on = 1;
        PSK_TRY(env_choice(ctx, "PSK_CX_PC_FILTER", {0, 1}, &pc_on));
        CxPlanKey key;
        key.M = a.M; key.n_ov = x.n_ov; key.cap = scan_grid_cap(ctx); key.side_cap = cx_side_grid_cap(ctx);
        key.pc_cap = cx_pc_grid_cap(ctx); key.pc_filter = pc_on;
        memcpy(&key.thr_bits, &a.cut.thr, 8);
        key.n1 = a.cut.n1; key.n0 = a.cut.n0; key.n_samples = ctx->n_samples;
        key.min_samples = a.cut.min_samples; key.max_samples = a.cut.max_samples; key.side_kernel = side_on;
        CxPlan &pl = ctx->cx_plan;
        if (!pl.valid || !(pl.key == key)) {
            pl.valid = false;
            cx_plan(a.cut.n1, a.cut.n0, ctx->n_samples, a.cut.min_samples, a.cut.max_samples, a.cut.thr, &pl.class_mask, pl.corner);
            pl.side = side_on && pl.class_mask == 0;
            uint64_t rows_per_block;
            pl.filtered = false;
            pl.rows_feasible = x.n_ov;
            pl.feas[0] = pl.feas[1] = pl.feas[2] = pl.feas[3] = ~0ull;
            if (pl.side && pc_on) {
                cx_pc_plan(a.cut.n1, a.cut.n0, ctx->n_samples, a.cut.min_samples, a.cut.max_samples, a.cut.thr, pl.feas);
                pl.rows_feasible = 0;
                for (size_t pc = 0; pc < ctx->cx_pc_hist.size() && pc < 256; pc++)
                    if ((pl.feas[pc >> 6] >> (pc & 63)) & 1ull) pl.rows_feasible += ctx->cx_pc_hist[pc];
                pl.filtered = pl.rows_feasible < x.n_ov;
#ifdef PSK_CX_PC_FORCE   // A/B builds: the filtered form whatever the count (the all-feasible comparison of the r15 table)
                pl.filtered = true;
#endif
            }
            if (pl.filtered) {
                const cx_side_shape_t sh = cx_pc_shape(x.n_ov, key.pc_cap);
                pl.grid = sh.blocks; pl.slot_blocks = 0; pl.ov_blocks = sh.blocks;
                rows_per_block = sh.rows_per_block;
            } else if (pl.side) {
                const cx_side_shape_t sh = cx_side_shape(x.n_ov, CL.cpr, key.side_cap);
                pl.grid = sh.blocks; pl.slot_blocks = 0; pl.ov_blocks = sh.blocks;
                rows_per_block = sh.rows_per_block;
            } else {
                x.class_mask = pl.class_mask;
                pl.grid = cx_grid(ctx, x, CL.cpr).x;
                pl.slot_blocks = x.slot_blocks; pl.ov_blocks = x.ov_blocks;
                rows_per_block = cx_rows_per_block(x, CL.cpr);
            }
            pl.seg_cap = result_seg_cap(dim3(pl.grid), rows_per_block);
            pl.key = key;
            pl.valid = true;
        }
        x.class_mask = pl.class_mask; x.corner[0] = pl.corner[0]; x.corner[1] = pl.corner[1];
        x.slot_blocks = pl.slot_blocks; x.ov_blocks = pl.ov_blocks;
        CL.grid = dim3(pl.grid);
        CL.side_kernel = pl.side;
        CL.filtered = pl.filtered;
        ctx->cx_last_plan = true;
        ctx->cx_last_filtered = pl.filtered;
        ctx->cx_last_rows_feasible = pl.rows_feasible;
        ctx->cx_last_class_mask = pl.class_mask;
        ctx->cx_last_skipped = pl.slot_blocks == 0;
        PSK_TRY(bind_results(ctx, a.sink, pl.seg_cap, set));
        if (pl.side) {
            CxSideArgs &sd = CL.side.s;
            CL.side.ov_pc = ctx->cx_ov_pc.as<uint16_t>();
            memcpy(CL.side.feas, pl.feas, sizeof(CL.side.feas));
            sd.ov = x.ov; sd.ov_row = x.ov_row; sd.n_ov = x.n_ov;
            memcpy(sd.m1, a.m1_inl, sizeof(sd.m1));
            memcpy(sd.m0, a.m0_inl, sizeof(sd.m0));
            sd.cut = a.cut;
            sd.sink = a.sink;
        }
        return PSK_OK;
    }
    PSK_TRY(pick_chi2_mode(ctx, L.weighted, a.cut.pcut, a.cut.pcut_bonf, a.cut.omit_B, &CL.mode));
    CL.grid = sh.grid;
    return setup_results(ctx, a, CL.grid, group_lanes(a), sh.unroll, set, sh.threads);
}

// Launches the scan and returns without waiting; psk_scan_end collects it.  Lets a caller queue other work (the
// survivor exchange of the previous scan) while the kernel streams the matrix.
static int chi2_scan_launch(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples, int max_samples,
                            double pvalue_cutoff, int omit_B, uint64_t n_kmers_global, bool keep_results)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->n_in_flight >= 2) return psk_fail(ctx, PSK_ESTATE, "two scans are in flight (psk_scan_end first)");
    if (!ctx->have_presence) return psk_fail(ctx, PSK_ESTATE, "no presence matrix (psk_build_presence first)");
    if (!pheno) return psk_fail(ctx, PSK_EINVAL, "null phenotype vector");
    if (n_kmers_global == 0) n_kmers_global = ctx->n_kmers ? ctx->n_kmers : 1;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int N = ctx->n_samples, wpr = mask_words(ctx);   // masks and tables: whole 16-byte chunks, also for 8-byte rows
    // one pinned staging block [m1 | m0 | w1 | w0] and ONE stream-ordered upload (weights only when given)
    const size_t n_mask = 2 * (size_t)wpr, n_w = 2 * (size_t)wpr * 64;
    const size_t stage_bytes = (n_mask + n_w) * 8;
    int set = 0;
    PSK_TRY(pick_result_set(ctx, &set, keep_results));
    if (2 * stage_bytes > ctx->scan_pinned_cap) {  // one staging block per result set: an upload may still be queued
        if (ctx->n_in_flight) PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->scan_pinned) (void)hipHostFree(ctx->scan_pinned);
        ctx->scan_pinned = nullptr;
        ctx->scan_pinned_cap = 0;
        PSK_HIP(ctx, hipHostMalloc(&ctx->scan_pinned, 2 * stage_bytes, hipHostMallocDefault));
        ctx->scan_pinned_cap = 2 * stage_bytes;
    }
    uint64_t *m1 = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(ctx->scan_pinned) + set * stage_bytes), *m0 = m1 + wpr;
    double *w = reinterpret_cast<double *>(m1 + n_mask);
    memset(m1, 0, weights ? stage_bytes : n_mask * 8);
    double W1 = 0, W0 = 0;
    int n1 = 0, n0 = 0;
    for (int i = 0; i < N; i++) {
        const double wi = weights ? weights[i] : 1.0;
        if (pheno[i] == 1) { m1[i >> 6] |= 1ull << (i & 63); if (weights) w[2 * (size_t)i] = wi; W1 += wi; n1++; }
        else if (pheno[i] == 0) { m0[i >> 6] |= 1ull << (i & 63); if (weights) w[2 * (size_t)i + 1] = wi; W0 += wi; n0++; }
    }
    // up to 1024 samples: the masks ride in the kernel arguments and an unweighted scan uploads nothing
    ctx->last.inline_masks = wpr <= SC_INL_WORDS ? 1 : 0;
    if (ctx->last.inline_masks) {
        memset(ctx->last.m1, 0, sizeof(ctx->last.m1));
        memset(ctx->last.m0, 0, sizeof(ctx->last.m0));
        memcpy(ctx->last.m1, m1, (size_t)wpr * 8);
        memcpy(ctx->last.m0, m0, (size_t)wpr * 8);
    }
    PSK_TRY(dev_reserve(ctx, ctx->mask1, stage_bytes));
    if (weights || !ctx->last.inline_masks)
        PSK_HIP(ctx, hipMemcpyAsync(ctx->mask1.p, m1, weights ? stage_bytes : n_mask * 8, hipMemcpyHostToDevice, ctx->stream));

    ctx->last.valid = true;
    ctx->last.weighted = weights != nullptr;
    ctx->last.min_samples = min_samples;
    ctx->last.max_samples = max_samples;
    ctx->last.pvalue_cutoff = pvalue_cutoff;
    ctx->last.omit_B = omit_B ? 1 : 0;
    ctx->last.n_kmers_global = n_kmers_global;
    ctx->last.n1 = n1; ctx->last.n0 = n0; ctx->last.W1 = W1; ctx->last.W0 = W0;
    Chi2Launch CL;
    PSK_TRY(fill_chi2_args(ctx, CL, set, true));
    ctx->last_scan_kind = 1;
    if (ctx->n_kmers) {
        ScanSlot &sl = ctx->slot[set];
        launch_chi2_any(ctx, CL, {sl.ev0, sl.ev1});   // the events ride on the dispatch: one command per scan
        PSK_HIP(ctx, hipGetLastError());
        sl.in_flight = true;
        sl.seq = ++ctx->scan_seq;
        ctx->n_in_flight++;
    } else {  // nothing to scan: an empty result, at once
        ctx->n_pass = 0;
        ctx->seg_counts.assign(SC_NSEG, 0);
        ctx->res_set = set;
        ctx->results_valid = true;
    }
    return PSK_OK;
}

extern "C" int psk_chi2_scan_begin(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples,
                                   int max_samples, double pvalue_cutoff, int omit_B, uint64_t n_kmers_global)
{
    return chi2_scan_launch(ctx, pheno, weights, min_samples, max_samples, pvalue_cutoff, omit_B, n_kmers_global, true);
}

extern "C" int psk_scan_end(psk_ctx *ctx, uint64_t *n_pass)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->n_in_flight) {  // the oldest scan in flight
        PSK_HIP(ctx, hipSetDevice(ctx->device));
        int set = ctx->slot[0].in_flight ? 0 : 1;
        if (ctx->slot[0].in_flight && ctx->slot[1].in_flight && ctx->slot[1].seq < ctx->slot[0].seq) set = 1;
        ScanSlot &sl = ctx->slot[set];
        PSK_HIP(ctx, hipEventSynchronize(sl.ev1));  // its kernels have written the counts to pinned memory
        sl.in_flight = false;
        ctx->n_in_flight--;
        float ms = 0;
        PSK_HIP(ctx, hipEventElapsedTime(&ms, sl.ev0, sl.ev1));
        ctx->last_scan_ms = ms;
        PSK_TRY(fetch_counts(ctx, set));
        ctx->dense_hint = ctx->n_pass * 1000 > ctx->n_kmers ? 1 : 0;  // only chi2 scans come through here
    }
    if (n_pass) *n_pass = ctx->n_pass;
    return PSK_OK;
}

extern "C" int psk_chi2_scan(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples,
                             int max_samples, double pvalue_cutoff, int omit_B, uint64_t n_kmers_global,
                             uint64_t *n_pass)
{
    if (ctx && ctx->n_in_flight) return psk_fail(ctx, PSK_ESTATE, "a scan is in flight (psk_scan_end first)");
    PSK_TRY(chi2_scan_launch(ctx, pheno, weights, min_samples, max_samples, pvalue_cutoff, omit_B, n_kmers_global, false));
    return psk_scan_end(ctx, n_pass);
}


static int rescan(psk_ctx *ctx, int reps, double *mean_ms, double *ms_each)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->n_in_flight) return psk_fail(ctx, PSK_ESTATE, "a scan is in flight (psk_scan_end first)");
    if (!ctx->have_presence || !ctx->last.valid || ctx->last_scan_kind != 1)
        return psk_fail(ctx, PSK_ESTATE, "no chi2 scan to repeat");
    if (reps < 1) return psk_fail(ctx, PSK_EINVAL, "reps must be >= 1");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    int set = 0;
    PSK_TRY(pick_result_set(ctx, &set));
    Chi2Launch CL;
    PSK_TRY(fill_chi2_args(ctx, CL, set, false));
    double ms = 0;
    PSK_TRY(run_chi2(ctx, CL, reps, &ms, ms_each));
    ctx->last_scan_ms = ms / reps;
    PSK_TRY(fetch_counts(ctx, set));
    if (mean_ms) *mean_ms = ms / reps;
    return PSK_OK;
}

extern "C" int psk_rescan_timed(psk_ctx *ctx, int reps, double *mean_ms) { return rescan(ctx, reps, mean_ms, nullptr); }

extern "C" int psk_rescan_times(psk_ctx *ctx, int reps, double *ms_each)
{
    if (ctx && !ms_each) return psk_fail(ctx, PSK_EINVAL, "null output array");
    return rescan(ctx, reps, nullptr, ms_each);
}

extern "C" int psk_chi2_pretest(double A, double B, double C, double D, double thr) { return chi2_pretest(A, B, C, D, thr) ? 1 : 0; }

extern "C" int psk_cx_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint32_t *class_mask,
                           uint64_t *corner)
{
    if (n1 < 0 || n0 < 0 || n_samples < 0 || n1 + n0 > n_samples || !class_mask || !corner) return PSK_EINVAL;
    cx_plan(n1, n0, n_samples, min_samples, max_samples, thr, class_mask, corner);
    return PSK_OK;
}

extern "C" int psk_cx_side_shape(uint64_t n_ov, int cpr, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block, uint32_t *batch_rows)
{
    if ((cpr != 1 && cpr != 2) || cap_blocks < 1 || cap_blocks > 0xffffffffull || !blocks || !rows_per_block) return PSK_EINVAL;
    const cx_side_shape_t sh = cx_side_shape(n_ov, cpr, cap_blocks);
    *blocks = sh.blocks;
    *rows_per_block = sh.rows_per_block;
    if (batch_rows) *batch_rows = sh.batch_rows;
    return PSK_OK;
}

extern "C" int psk_cx_pc_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint64_t *feas)
{
    if (n1 < 0 || n0 < 0 || n_samples < 0 || n_samples > CX_MAX_SAMPLES || n1 + n0 > n_samples || !feas) return PSK_EINVAL;
    cx_pc_plan(n1, n0, n_samples, min_samples, max_samples, thr, feas);
    return PSK_OK;
}

extern "C" int psk_cx_pc_shape(uint64_t n_ov, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block, uint32_t *batch_rows)
{
    if (cap_blocks < 1 || cap_blocks > 0xffffffffull || !blocks || !rows_per_block) return PSK_EINVAL;
    const cx_side_shape_t sh = cx_pc_shape(n_ov, cap_blocks);
    *blocks = sh.blocks;
    *rows_per_block = sh.rows_per_block;
    if (batch_rows) *batch_rows = sh.batch_rows;
    return PSK_OK;
}

extern "C" int psk_last_scan_filter(const psk_ctx *ctx, int *filtered, uint64_t *rows_feasible, uint64_t *rows_overflow)
{
    if (!ctx) return PSK_EINVAL;
    if (filtered) *filtered = ctx->cx_last_plan && ctx->cx_last_filtered ? 1 : 0;
    if (rows_feasible) *rows_feasible = ctx->cx_last_plan ? ctx->cx_last_rows_feasible : 0;
    if (rows_overflow) *rows_overflow = ctx->cx_last_plan ? ctx->cx_n_ov : 0;
    return PSK_OK;
}

extern "C" int psk_last_scan_plan(const psk_ctx *ctx, int *encoded, uint32_t *class_mask, int *slots_skipped)
{
    if (!ctx) return PSK_EINVAL;
    if (encoded) *encoded = ctx->cx_last_plan ? 1 : 0;
    if (class_mask) *class_mask = ctx->cx_last_plan ? ctx->cx_last_class_mask : 0;
    if (slots_skipped) *slots_skipped = ctx->cx_last_plan && ctx->cx_last_skipped ? 1 : 0;
    return PSK_OK;
}
