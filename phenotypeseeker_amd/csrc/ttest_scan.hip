// The Welch scan (ttest_scan_kernel replaces conduct_t_test / get_samples_distribution_for_ttest, modeling.py:716-757)
// and the tables of the moment scans: the two table-building kernels and their host side, for this scan and for the
// weighted chi2 scan (assoc_scan.hip).  The row stream and the lane-per-row moment forms are scan_common.h's.
// Compiled with -ffp-contract=off: the exact pass evaluates the reference's operations in the reference's order.
#include "scan_common.h"

#include <algorithm>
#include <cmath>

namespace {

// ---- Student-t two-sided p-value: I_{df/(df+t^2)}(df/2, 1/2), Lentz continued fraction ---------
__device__ double dev_betacf(double a, double b, double x)
{
    const double TINY = 1e-300, EPS = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < TINY) d = TINY;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 10000; m++) {
        const int m2 = 2 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < TINY) d = TINY;
        c = 1.0 + aa / c; if (fabs(c) < TINY) c = TINY;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < TINY) d = TINY;
        c = 1.0 + aa / c; if (fabs(c) < TINY) c = TINY;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < EPS) break;
    }
    return h;
}

__device__ double dev_betainc(double a, double b, double x)
{
    if (!(x > 0.0)) return (x == 0.0) ? 0.0 : NAN;
    if (!(x < 1.0)) return (x == 1.0) ? 1.0 : NAN;
    const double lbt = lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log1p(-x);
    const double bt = exp(lbt);
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * dev_betacf(a, b, x) / a;
    return 1.0 - bt * dev_betacf(b, a, 1.0 - x) / b;
}

__device__ __attribute__((noinline)) double dev_t_two_sided_p(double t, double df)
{
    if (isnan(t) || isnan(df) || !(df > 0)) return NAN;
    if (isinf(t)) return 0.0;
    return dev_betainc(0.5 * df, 0.5, df / (df + t * t));
}

// Welch scan.  Phase A is the chi2 kernel's streaming shape (one 16-byte load per lane per row, popcount
// against the non-NA mask, group reduce, frequency filter of modeling.py:731).  Rows that pass are queued
// per wave and handled 64 at a time, one row per lane (row_moments): ONE pass of (weighted) moments of the
// k-mer-present group over phenotype values shifted by their global weighted mean -- the absent group
// follows from the totals -- then means, variances, t and the Satterthwaite df in the same lane.
// Table layout: unit weights tab[s] = {u, u*u} (n comes from the popcount); GSC weights {w, w*u, w*u*u};
// zeros for NA samples and padding.
template <int G, bool WT, bool LUT = false, bool F32 = false>
__global__ __launch_bounds__(LUT ? SC_LUT_THREADS : SC_THREADS) void ttest_scan_kernel(const ScanArgs P, const double mu)
{
    constexpr bool HALF = G == 0;          // 8-byte rows, two per load
    constexpr int THREADS = sc_threads<G, LUT>(), UNR = sc_unroll<G, LUT>();
    __shared__ uint64_t s_qrow[THREADS / 64][rq_cap(G, UNR)];
    __shared__ int2 s_qval[THREADS / 64][rq_cap(G, UNR)];
    constexpr int NM = WT ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) double s_lut[];   // LUT: the nibble table of row_moments_lut / the six-bit f32 table
    if (LUT && F32) load_lut(s_lut, reinterpret_cast<const double *>(P.lut6), (int)(lut6_bytes(P.cpr, NM) / 8), THREADS);
    else if (LUT) load_lut(s_lut, P.lut, P.c_lut * 32 * 16 * NM, THREADS);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int g = lane & (sc_lanes(G) - 1);
    RowMasks<1> mk = {{0}, {0}, {P.mvalid}};   // the non-NA samples
    if (g < P.cpr) { mk.a[0] = P.mvalid[2 * g]; mk.b[0] = P.mvalid[2 * g + 1]; }
    RowQueue Q = {s_qrow[wid], s_qval[wid], 0};

    auto process = [&](int cnt) {
        const bool act = lane < cnt;
        const uint64_t r = Q.row[act ? lane : 0];
        const int r_nw = Q.val[act ? lane : 0].x;
        double mo[NM];
        if (F32) row_moments_f32<NM, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, reinterpret_cast<const float *>(s_lut), mo);
        else if (LUT) row_moments_mixed<NM, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, P.c_lut, s_lut, (cdptr)P.tab, mo);
        else row_moments<NM, HALF>(sc_row_ptr<HALF>(P, r), P.cpr, (cdptr)P.tab, mo);
        if (!act) return;
        const double nx = WT ? mo[0] : (double)r_nw, sx = mo[NM - 2], qx = mo[NM - 1];
        const double ny = P.W1 - nx, sy = P.W0 - sx, qy = P.cut.thr - qx;  // totals: W1 = sum w, W0 = sum w*u, thr = sum w*u^2
        if (F32) {
            // the sums are f32 sums, off by at most e0 (sum w; 0 with unit weights: the popcount), e1 (sum w u), e2 (sum w u^2):
            // an UPPER bound of |t| -- the largest difference of the means over the smallest standard error the bounds
            // allow -- decides who is a candidate (ttest_finalize_kernel computes the statistic itself)
            const double e0 = WT ? P.e0 : 0.0;
            const double nxl = nx - e0, nyl = ny - e0, nxh = nx + e0, nyh = ny + e0;
            bool cand = !(nxl > 1.0 && nyl > 1.0);
            if (!cand) {
                const double ax = fabs(sx) + P.e1, ay = fabs(sy) + P.e1;
                // (+ 2 eref: the exact pass reproduces the reference's sums of the RAW values, whose means are only good to
                // ~n eps max|v| -- a phenotype of 1e6 +- 1e-3 makes that visible in t, and such a row must still be offered)
                const double dmax = fabs(sx / nx - sy / ny) + P.e1 * (1.0 / nxl + 1.0 / nyl) + ax * e0 / (nxl * nxl) + ay * e0 / (nyl * nyl) + 2.0 * P.eref;
                const double vx = fmax((qx - P.e2) - ax * ax / nxl, 0.0) / nxh, vy = fmax((qy - P.e2) - ay * ay / nyl, 0.0) / nyh;
                const double sem = vx / (nxh - 1.0) + vy / (nyh - 1.0);
                cand = !(sem > 0.0) || !(dmax / sqrt(sem) <= P.tcrit);
            }
            if (cand) append_candidate(P.sink, r, r_nw);
            return;
        }
        const double dx = sx / nx, dy = sy / ny;              // group means minus mu
        const double vx = (qx - sx * dx) / nx, vy = (qy - sy * dy) / ny;  // ddof = 0
        const double sem1 = vx / (nx - 1.0), sem2 = vy / (ny - 1.0);
        const double semsum = sem1 + sem2;
        const double tstat = (dx - dy) / sqrt(semsum);
        // Student's t has heavier tails than the normal, p_t >= erfc(|t|/sqrt 2): rows with
        // |t| <= t_crit (erfc(t_crit/sqrt 2) = cut, solved on the host, less a margin far above the ~1e-15 by which these
        // sums differ from the sample-order ones) cannot pass.  Candidates are stored as (row, n_with) only:
        // ttest_finalize_kernel sums their moments again in the reference's order and decides (keeps erfc /
        // incomplete-beta code, and its ~90 VGPRs, out of this kernel).
        if (!(fabs(tstat) + 2.0 * P.eref / sqrt(semsum) <= P.tcrit)) append_candidate(P.sink, r, r_nw);   // eref: see ScanArgs; NaN: the exact pass drops it
    };

    auto on_row = [&](uint64_t row, const uint32_t (&cnt)[1], bool lead) {
        const int n_w = (int)cnt[0], n_wo = P.nvalid - (int)cnt[0];
        const bool freq_ok = (row < P.M) && !(n_w < P.cut.min_samples || n_wo < 2 || n_w > P.cut.max_samples);
        Q.n = queue_rows(freq_ok && lead, row, make_int2(n_w, 0), Q.row, Q.val, Q.n, lane);
    };
    stream_rows<G, LUT>(P, mk, Q, on_row, process);
}

// Second pass of the Welch scan: one workgroup per result segment, one candidate per lane.  The candidate's moments are
// summed AGAIN in the reference's order -- conduct_t_test / get_samples_distribution_for_ttest (modeling.py:716-757)
// hand the two groups' values and weights, in sample order, to a weighted DescrStatsW: per group sum w and sum w v, the
// weighted mean, then sum w (v - mean)^2 (ddof = 0), std_meandiff_separatevar and the Satterthwaite df -- with every
// operation an IEEE double operation in that order (this file is compiled with -ffp-contract=off; a weight times 1.0 or
// 0.0 is exact, so `fma(present ? 1 : 0, term, acc)` IS the conditional addition), so t, the two means, round(t, 2)
// and the "%.2E" of the p-value follow from the same bits as a sample-order CPU evaluation (r02: moments from the scan kernel's nibble-table
// sums, ~1e-15 off, and up to two rows flipping at the cut).  Then the two-sided p, the keep rule p < cut / M
// (modeling.py:738) and the compaction of the segment in place.  Candidates are the rows whose scan-kernel |t| exceeds
// a bound no passing row can be under (psk_ttest_scan: t_crit), so the scan kernel's own sums decide nothing.
template <bool WT>
__global__ __launch_bounds__(SC_FIN_THREADS) void ttest_finalize_kernel(const ScanArgs P)
{
    __shared__ uint32_t scan_lds[SC_FIN_THREADS / 64];
    __shared__ uint32_t s_out;
    __shared__ double2 s_tab[SC_FIN_BLK * 128];   // pass 1: {weight, weight * value}, pass 2: {weight, value} of the samples of the current block (broadcast reads)
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
        // One lane walks its candidate's 2 x n_samples dependent additions (rocprof, r03: 82 us at 1,024 samples whatever the
        // number of candidates).  A weight times 1.0 or 0.0 is exact, so fma(present ? 1 : 0, term, acc) IS the conditional
        // addition; the product w v comes out of the staged table, and with unit weights the two weight sums are the counts
        // the scan kernel already has.  Tried and dropped (r03): a branch on the bit instead of the 0/1 factors (94 / 107 us:
        // both sides of a divergent branch issue), and chains of precomputed addends summed by one lane per chain (69 us per
        // two batches of four candidates, and any segment beyond the batches still pays the 82).
        double nx = 0.0, ny = 0.0, sx = 0.0, sy = 0.0, qx = 0.0, qy = 0.0, mx = 0.0, my = 0.0;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                if (!WT) { nx = (double)nw; ny = (double)(P.nvalid - nw); }   // sums of ones: exact
                mx = sx / nx; my = sy / ny;
            }
            for (int c0 = 0; c0 < P.cpr; c0 += SC_FIN_BLK) {
                const int nc = P.cpr - c0 < SC_FIN_BLK ? P.cpr - c0 : SC_FIN_BLK;
                __syncthreads();   // the previous block has been consumed
                for (int e = threadIdx.x; e < nc * 128; e += SC_FIN_THREADS) {
                    double2 t = reinterpret_cast<const double2 *>(P.raw)[(size_t)c0 * 128 + e];   // NA and padding: {0, 0}
                    if (pass == 0) t.y = t.x * t.y;
                    s_tab[e] = t;
                }
                __syncthreads();
                if (!wave_any) continue;
                // the row's chunks are requested two ahead: read where they are used, every 16-byte chunk cost this lone
                // lane a whole memory latency (16 of them per candidate at 1,024 samples: half of the kernel's 82 us)
                u32x4 y0 = P.half ? sc_ld_chunk<true>(rp, 0) : rp[c0], y1 = nc > 1 ? rp[c0 + 1] : (u32x4)(0u);   // (an 8-byte row: the table's samples 64 ... 127 are {0, 0})
                for (int ch = 0; ch < nc; ch++) {
                    const u32x4 y = y0;
                    y0 = y1;
                    if (ch + 2 < nc) y1 = rp[c0 + ch + 2];
                    const uint32_t w4[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                    for (int h = 0; h < 4; h++) {
#pragma unroll 8
                        for (int sb = 0; sb < 32; sb++) {
                            const uint32_t fh = (uint32_t)(((int32_t)(w4[h] << (31 - sb))) >> 31) & 0x3FF00000u;
                            const double f = __hiloint2double((int)fh, 0), g = __hiloint2double((int)(fh ^ 0x3FF00000u), 0);
                            const double2 t = s_tab[ch * 128 + h * 32 + sb];
                            if (pass == 0) {
                                if (WT) { nx = fma(f, t.x, nx); ny = fma(g, t.x, ny); }
                                sx = fma(f, t.y, sx);
                                sy = fma(g, t.y, sy);
                            } else {
                                const double d = t.y - (fh ? mx : my);
                                // unit weights: (1 d) d = d d; an NA sample (weight 0 in the table) adds nothing to either group
                                const double term = WT ? (t.x * d) * d : (t.x != 0.0 ? d * d : 0.0);
                                qx = fma(f, term, qx);
                                qy = fma(g, term, qy);
                            }
                        }
                    }
                }
            }
        }
        double tstat = 0.0, p = 1.0;
        bool keep = false;
        if (valid) {
            const double vx = qx / nx, vy = qy / ny;          // ddof = 0
            const double sem1 = vx / (nx - 1.0), sem2 = vy / (ny - 1.0);
            const double semsum = sem1 + sem2;
            tstat = (mx - my) / sqrt(semsum);
            const double z1 = (sem1 / semsum) * (sem1 / semsum) / (nx - 1.0);
            const double z2 = (sem2 / semsum) * (sem2 / semsum) / (ny - 1.0);
            p = dev_t_two_sided_p(tstat, 1.0 / (z1 + z2));
            keep = p < P.cut.pcut_bonf;
        }
        uint32_t tot;
        const uint32_t pos = psk_block_excl_scan_u32<SC_FIN_THREADS>(keep ? 1u : 0u, &tot, scan_lds);  // barriers inside
        const uint32_t out = s_out;
        if (keep) {
            const uint64_t o = base + out + pos;  // <= base + i: compaction only moves entries down
            P.sink.res_row[o] = row; P.sink.res_stat[o] = tstat; P.sink.res_p[o] = p; P.sink.res_mx[o] = mx; P.sink.res_my[o] = my; P.sink.res_nw[o] = nw;
        }
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

// np.add.reduce of a float64 stream of n values, fed in order: from 0.0, the pairwise sums (numpy's pairwise_sum:
// sequential from -0.0 below 8 elements, eight interleaved accumulators up to 128, else the two halves with the split
// rounded down to a multiple of 8) of its 8,192-element buffers in turn.  The tree of a buffer is walked leaf by leaf: a
// frame per level holds the size of the right half still to come (0 once it is under way) and the left half's sum.
struct NpSum {
    double tot, acc, r[8], left[8];
    int right[8], depth, leaf, k, rest;
};
__device__ int np_descend(NpSum &s, int sz)
{
    while (sz > 128) {
        int n2 = sz / 2;
        n2 -= n2 % 8;
        s.right[s.depth++] = sz - n2;
        sz = n2;
    }
    return sz;
}
__device__ void np_next_buffer(NpSum &s)
{
    const int c = s.rest < 8192 ? s.rest : 8192;
    s.rest -= c;
    s.depth = 0;
    s.leaf = np_descend(s, c);
    s.k = 0;
}
__device__ void np_begin(NpSum &s, int n)
{
    s.tot = 0.0;
    s.rest = n;
    if (n > 0) np_next_buffer(s);
}
__device__ double np_fold8(const double *r) { return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])); }
__device__ void np_add(NpSum &s, double v)
{
    const int L = s.leaf, body = L - L % 8;
    if (L < 8) s.acc = (s.k == 0 ? -0.0 : s.acc) + v;
    else if (s.k < 8) s.r[s.k] = v;
    else if (s.k < body) s.r[s.k & 7] += v;
    else {
        if (s.k == body) s.acc = np_fold8(s.r);
        s.acc += v;
    }
    if (++s.k < L) return;
    double sum = (L >= 8 && body == L) ? np_fold8(s.r) : s.acc;   // the leaf is done
    while (s.depth > 0) {
        const int t = s.depth - 1;
        if (s.right[t] > 0) {   // its left half: the right half comes next
            s.left[t] = sum;
            const int rs = s.right[t];
            s.right[t] = 0;
            s.leaf = np_descend(s, rs);
            s.k = 0;
            return;
        }
        sum = s.left[t] + sum;
        s.depth = t;
    }
    s.tot += sum;
    if (s.rest > 0) np_next_buffer(s);
}

// The two means of every Welch survivor as the reference prints them: np.average(x, weights=x_weights)
// (modeling.py:735-736) = the numpy sums of w v and of w over the group's samples in sample order.  ttest_finalize_kernel's
// t follows DescrStatsW's sums, which it adds in sample order; the two orders differ by an ulp now and then, and at a
// two-decimal tie that ulp decides round(mean, 2).  One thread per survivor (they are few), after the finalize kernel has
// compacted its segment.
template <bool WT>
__global__ __launch_bounds__(256) void ttest_means_kernel(const ScanArgs P)
{
    const uint32_t seg = blockIdx.x;
    const uint32_t c = min(P.sink.final_counts[seg], P.sink.seg_cap);   // (an overflowed segment is refused by fetch_counts)
    const uint64_t base = (uint64_t)seg * P.sink.seg_cap;
    const double2 *raw = reinterpret_cast<const double2 *>(P.raw);   // {weight, value}; NA: {0, 0}
    const int words = P.half ? 1 : 2 * P.cpr;
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
        const uint64_t row = P.sink.res_row[base + i];
        const int nw = P.sink.res_nw[base + i];
        const uint64_t *rp = reinterpret_cast<const uint64_t *>(P.bits) + row * (uint64_t)words;
        NpSum sx, sy, wx, wy;
        np_begin(sx, nw);
        np_begin(sy, P.nvalid - nw);
        if (WT) { np_begin(wx, nw); np_begin(wy, P.nvalid - nw); }
        for (int wd = 0; wd < words; wd++) {
            const uint64_t pres = rp[wd];
            for (uint64_t m = P.mvalid[wd]; m; m &= m - 1) {
                const int b = __ffsll((long long)m) - 1;
                const double2 t = raw[wd * 64 + b];
                if ((pres >> b) & 1) { np_add(sx, t.y * t.x); if (WT) np_add(wx, t.x); }
                else { np_add(sy, t.y * t.x); if (WT) np_add(wy, t.x); }
            }
        }
        P.sink.res_mx[base + i] = sx.tot / (WT ? wx.tot : (double)nw);
        P.sink.res_my[base + i] = sy.tot / (WT ? wy.tot : (double)(P.nvalid - nw));
    }
}

template <bool WT, bool LUT = false, bool F32 = false>
void launch_ttest_form(int G, dim3 grid, size_t lds, hipStream_t st, TimedBy ev, const ScanArgs &a, double mu)
{
    dispatch_G<LUT ? 16 : 64>(G, [&](auto g) {
        launch_timed(ttest_scan_kernel<decltype(g)::value, WT, LUT, F32>, grid, LUT ? SC_LUT_THREADS : SC_THREADS, lds, st, ev, a, mu);
    });
}

// (three kernels: the scan's time runs from the start of the first to the end of the third)
template <bool WT>
void launch_ttest_w(int G, dim3 grid, hipStream_t st, TimedBy ev, const ScanArgs &a, double mu)
{
    if (a.lut6) launch_ttest_form<WT, true, true>(G, grid, lut6_bytes(a.cpr, WT ? 3 : 2), st, ev.first(), a, mu);
    else if (a.lut) launch_ttest_form<WT, true>(G, grid, lut_bytes(a.c_lut, WT ? 3 : 2), st, ev.first(), a, mu);
    else launch_ttest_form<WT>(G, grid, 0, st, ev.first(), a, mu);
    launch_timed(ttest_finalize_kernel<WT>, dim3(SC_NSEG), SC_FIN_THREADS, 0, st, TimedBy(), a);
    launch_timed(ttest_means_kernel<WT>, dim3(SC_NSEG), 256, 0, st, ev.last(), a);
}

void launch_ttest(int G, dim3 grid, hipStream_t st, TimedBy ev, const ScanArgs &a, double mu, bool weighted)
{
    if (weighted) launch_ttest_w<true>(G, grid, st, ev, a, mu);
    else launch_ttest_w<false>(G, grid, st, ev, a, mu);
}

// builds the nibble table of row_moments_lut (scan_common.h)
template <int NM>
__global__ void moment_lut_kernel(const double *__restrict__ tab, int n_groups, double *__restrict__ lut)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_groups * 16) return;
    const int g = i >> 4, p = i & 15;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if ((p >> b) & 1) s += tab[(size_t)(4 * g + b) * NM + m];
        // NM = 3: the first two moments as 16-byte pairs, the third in a table of its own behind them (row_moments_lut)
        if (NM == 3) lut[m < 2 ? (size_t)i * 2 + m : (size_t)n_groups * 32 + i] = s;
        else lut[(size_t)i * NM + m] = s;
    }
}

// builds the six-bit f32 table of row_moments_f32 (scan_common.h)
template <int NM>
__global__ void moment_lut6_kernel(const double *__restrict__ tab, int chunks, float *__restrict__ lut)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= chunks * SC_L6_ENTRIES) return;
    const int ch = i / SC_L6_ENTRIES, e = i % SC_L6_ENTRIES;
    const int j = e < 21 * 64 ? e >> 6 : 21, p = e < 21 * 64 ? e & 63 : e - 21 * 64, width = j < 21 ? 6 : 2;
    const size_t s0 = (size_t)ch * 128 + 6 * j;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        double s = 0.0;
        for (int b = 0; b < width; b++)
            if ((p >> b) & 1) s += tab[(s0 + b) * NM + m];
        if (m < 2) lut[(size_t)i * 2 + m] = (float)s;
        else lut[(size_t)chunks * SC_L6_ENTRIES * 2 + i] = (float)s;
    }
}

}  // namespace

// chunks of a row that go through the table: all of them when the table fits the LDS (up to 1536 samples with two
// moments, 1024 with three), else as many as fit -- the rest of the row takes the per-sample form (row_moments_mixed);
// 0 = the per-sample kernels (PSK_NO_LUT, or rows wider than 16 lanes)
static int lut_chunks(int cpr, int nm)
{
    if (env_flag("PSK_NO_LUT") || cpr > 16) return 0;
    int c = env_flag("PSK_LUT_HALF") ? (cpr + 1) / 2 : cpr;
    while (c > 0 && lut_bytes(c, nm) > SC_LUT_MAX_BYTES) c--;
    return c;
}

// builds the nibble table of `tab` (cpr * 128 samples x nm moments, already on the device) into ctx->lut
static int build_moment_lut(psk_ctx *ctx, const double *tab, int chunks, int nm)
{
    const int n_groups = chunks * 32;
    PSK_TRY(dev_reserve(ctx, ctx->lut, lut_bytes(chunks, nm)));
    if (nm == 2) moment_lut_kernel<2><<<div_up((uint64_t)n_groups * 16, 256), 256, 0, ctx->stream>>>(tab, n_groups, ctx->lut.as<double>());
    else moment_lut_kernel<3><<<div_up((uint64_t)n_groups * 16, 256), 256, 0, ctx->stream>>>(tab, n_groups, ctx->lut.as<double>());
    PSK_HIP(ctx, hipGetLastError());
    return PSK_OK;
}

// the six-bit f32 table of `tab` for a whole row (cpr chunks), when it fits the LDS beside the kernels' queues; PSK_LUT_F64
// keeps the nibble table in f64 (A/B runs).  *built = false: not this time.
static int build_moment_lut6(psk_ctx *ctx, const double *tab, int cpr, int nm, bool *built)
{
    *built = false;
    if (env_flag("PSK_NO_LUT") || env_flag("PSK_LUT_F64") || cpr > 16 || lut6_bytes(cpr, nm) > SC_LUT_MAX_BYTES) return PSK_OK;
    PSK_TRY(dev_reserve(ctx, ctx->lut, lut6_bytes(cpr, nm)));
    const int n = cpr * SC_L6_ENTRIES;
    if (nm == 2) moment_lut6_kernel<2><<<div_up((uint64_t)n, 256), 256, 0, ctx->stream>>>(tab, cpr, ctx->lut.as<float>());
    else moment_lut6_kernel<3><<<div_up((uint64_t)n, 256), 256, 0, ctx->stream>>>(tab, cpr, ctx->lut.as<float>());
    PSK_HIP(ctx, hipGetLastError());
    *built = true;
    return PSK_OK;
}
// (additions per accumulator + rounding of the entry and of the final sums) x 2^-24, with room: what an f32 sum of
// row_moments_f32 may be off by, relative to the sum of the absolute values of ALL the terms of the table
static double lut6_gamma(int cpr) { return ((double)(cpr * 22) / 2.0 + 8.0) * 5.9604644775390625e-08 * 1.01; }

// The table of a moment scan and what goes with it, for both scans.  `tab`: the per-sample table on the device (a.cpr
// chunks x 128 samples x nm moments); build = false: the table the last scan left in ctx->lut (a repeated scan).  The
// six-bit f32 table when a row's fits, else the f64 nibble table of as many chunks as fit (lut_chunks), else none.
// s0, s1, s2: the sums of the absolute terms of the moments, which the error bounds of the f32 sums scale with
// (row_moments_f32; chi2: the two class weight totals).  tab == nullptr: a scan without moments.
// Returns the launch shape; the caller's setup_results call follows.
int setup_table_scan(psk_ctx *ctx, ScanArgs &a, const double *tab, int nm, double s0, double s1, double s2, bool build, ScanShape *sh)
{
    if (build) {
        ctx->lut_valid = ctx->lut6_valid = false;   // the table buffer is shared by the moment scans
        if (tab) PSK_TRY(build_moment_lut6(ctx, tab, a.cpr, nm, &ctx->lut6_valid));
        if (tab && !ctx->lut6_valid && lut_chunks(a.cpr, nm) > 0) {
            PSK_TRY(build_moment_lut(ctx, tab, lut_chunks(a.cpr, nm), nm));
            ctx->lut_valid = true;
        }
    }
    a.lut6 = (tab && ctx->lut6_valid) ? ctx->lut.as<float>() : nullptr;
    a.lut = (tab && ctx->lut_valid && !a.lut6) ? ctx->lut.as<double>() : nullptr;
    a.c_lut = a.lut ? lut_chunks(a.cpr, nm) : 0;
    if (a.lut6) {   // what the f32 sums of the candidate pass may be off by (row_moments_f32)
        const double gm = lut6_gamma(a.cpr);
        a.e0 = gm * s0 + 1e-36; a.e1 = gm * s1 + 1e-36; a.e2 = gm * s2 + 1e-36;
    }
    const bool table = a.lut != nullptr || a.lut6 != nullptr;
    const int G = group_lanes(a);
    sh->grid = scan_grid(ctx, a.M, G, SC_UNROLL, table);
    sh->unroll = table ? lut_unroll(G) : SC_UNROLL;
    sh->threads = table ? SC_LUT_THREADS : SC_THREADS;
    return PSK_OK;
}

namespace {
// What the host makes of a Welch scan's phenotype: the non-NA mask, the table of the kernel's moments and, behind it, the
// {weight, value} pairs of the exact pass; the totals the absent group follows from and the bounds scale with.
struct WelchTables {
    std::vector<uint64_t> mv;   // non-NA mask
    std::vector<double> vw;     // row_moments table: {u, u^2} or {w, w u, w u^2} per sample; from raw_off: {weight, value}
    size_t raw_off = 0;
    bool unit_w = true;
    int NM = 2, nvalid = 0;
    double mu = 0.0, scale = 1.0;
    double tot_w = 0.0, tot_wu = 0.0, tot_wuu = 0.0, abs_wu = 0.0, max_abs_v = 0.0;
};
}  // namespace

static WelchTables welch_tables(const double *pheno, const uint8_t *valid, const double *weights, int N, int wpr)
{
    WelchTables T;
    T.mv.assign(wpr, 0);
    for (int i = 0; weights && i < N; i++) if (valid[i] && weights[i] != 1.0) T.unit_w = false;
    T.NM = T.unit_w ? 2 : 3;
    T.raw_off = (size_t)T.NM * wpr * 64;             // the exact pass's {weight, value} pairs follow the moment table
    T.vw.assign(T.raw_off + (size_t)2 * wpr * 64, 0.0);
    double sw = 0.0, swv = 0.0;
    for (int i = 0; i < N; i++) {
        if (!valid[i]) continue;
        const double wi = weights ? weights[i] : 1.0;
        sw += wi;
        swv += wi * pheno[i];
    }
    const double mu = T.mu = sw > 0 ? swv / sw : 0.0;  // the kernel accumulates moments of (value - mu)
    // ... scaled by a power of two (exact; t does not change) so that the spread is ~1: the f32 table of the candidate
    // pass then neither underflows nor overflows whatever unit the phenotype is in
    double &scale = T.scale;
    {
        double ss = 0.0;
        for (int i = 0; i < N; i++) if (valid[i]) { const double u = pheno[i] - mu; ss += (weights ? weights[i] : 1.0) * u * u; }
        const double sd = sw > 0 ? std::sqrt(ss / sw) : 0.0;
        if (sd > 0 && std::isfinite(sd)) { int ex = 0; (void)std::frexp(sd, &ex); scale = std::ldexp(1.0, 1 - ex); }
    }
    std::vector<double> &vw = T.vw;
    for (int i = 0; i < N; i++) {
        if (!valid[i]) continue;
        T.mv[i >> 6] |= 1ull << (i & 63);
        const double u = (pheno[i] - mu) * scale, wi = weights ? weights[i] : 1.0;
        T.abs_wu += std::fabs(wi * u);
        T.max_abs_v = std::max(T.max_abs_v, std::fabs(pheno[i]));
        if (T.unit_w) { vw[2 * (size_t)i] = u; vw[2 * (size_t)i + 1] = u * u; }
        else { vw[3 * (size_t)i] = wi; vw[3 * (size_t)i + 1] = wi * u; vw[3 * (size_t)i + 2] = wi * u * u; }
        T.tot_w += wi; T.tot_wu += wi * u; T.tot_wuu += wi * u * u;
        vw[T.raw_off + 2 * (size_t)i] = wi; vw[T.raw_off + 2 * (size_t)i + 1] = pheno[i];
        T.nvalid++;
    }
    return T;
}

// t_crit: erfc(t_crit / sqrt 2) = cut by bisection (-1 when everything may pass)
static double welch_tcrit(double cut)
{
    double lo = 0.0, hi = 40.0;
    if (!(cut < 1.0)) hi = 0.0;
    else if (std::erfc(hi * 0.70710678118654752440) >= cut) lo = hi;  // cut below double's erfc range
    else
        for (int it = 0; it < 200; it++) {
            const double mid = 0.5 * (lo + hi);
            if (std::erfc(mid * 0.70710678118654752440) >= cut) lo = mid; else hi = mid;
        }
    return cut < 1.0 ? lo * (1.0 - 1e-9) : -1.0;  // err on the side of keeping candidates (the exact pass decides)
}

extern "C" int psk_ttest_scan(psk_ctx *ctx, const double *pheno, const uint8_t *valid, const double *weights,
                              int min_samples, int max_samples, double pvalue_cutoff, uint64_t n_kmers_global,
                              uint64_t *n_pass)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->n_in_flight) return psk_fail(ctx, PSK_ESTATE, "a scan is in flight (psk_scan_end first)");
    if (!ctx->have_presence) return psk_fail(ctx, PSK_ESTATE, "no presence matrix (psk_build_presence first)");
    if (!pheno || !valid) return psk_fail(ctx, PSK_EINVAL, "null phenotype vector");
    if (n_kmers_global == 0) n_kmers_global = ctx->n_kmers ? ctx->n_kmers : 1;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const int N = ctx->n_samples, wpr = mask_words(ctx);   // masks and tables: whole 16-byte chunks, also for 8-byte rows
    const WelchTables T = welch_tables(pheno, valid, weights, N, wpr);
    PSK_TRY(dev_reserve(ctx, ctx->mask1, wpr * 8));
    PSK_TRY(dev_reserve(ctx, ctx->phe, T.vw.size() * 8));
    PSK_HIP(ctx, hipMemcpyAsync(ctx->mask1.p, T.mv.data(), wpr * 8, hipMemcpyHostToDevice, ctx->stream));
    PSK_HIP(ctx, hipMemcpyAsync(ctx->phe.p, T.vw.data(), T.vw.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ScanArgs a = ScanArgs();
    a.bits = reinterpret_cast<const u32x4 *>(ctx->bits.p);
    a.M = ctx->n_kmers;
    a.cpr = wpr / 2;
    a.half = ctx->wpr == 1;
    a.mvalid = ctx->mask1.as<uint64_t>();
    a.tab = ctx->phe.as<double>();
    a.raw = a.tab + T.raw_off;
    a.nvalid = T.nvalid;
    a.cut.min_samples = min_samples;
    a.cut.max_samples = max_samples;
    a.cut.pcut = pvalue_cutoff;
    a.cut.pcut_bonf = pvalue_cutoff / (double)n_kmers_global;
    a.W1 = T.tot_w; a.W0 = T.tot_wu; a.cut.thr = T.tot_wuu;  // totals over the non-NA samples (shifted values)
    a.tcrit = welch_tcrit(a.cut.pcut_bonf);
    int set = 0;
    PSK_TRY(pick_result_set(ctx, &set));
    a.eref = 4.0 * (double)N * 1.1102230246251565e-16 * T.max_abs_v * T.scale;   // in the kernel's (shifted, scaled) units
    ScanShape sh;
    PSK_TRY(setup_table_scan(ctx, a, a.tab, T.NM, T.tot_w, T.abs_wu, T.tot_wuu, true, &sh));
    const int G = group_lanes(a);
    PSK_TRY(setup_results(ctx, a, sh.grid, G, sh.unroll, set, sh.threads));
    ctx->n_pass = 0;
    ctx->last_scan_kind = 2;
    ctx->last.valid = false;
    if (ctx->n_kmers) {
        launch_ttest(G, sh.grid, ctx->stream, {ctx->ev0, ctx->ev1}, a, T.mu, !T.unit_w);
        PSK_HIP(ctx, hipGetLastError());
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0;
        PSK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->last_scan_ms = ms;
        PSK_TRY(fetch_counts(ctx, set));
    } else {
        ctx->seg_counts.assign(SC_NSEG, 0);
        ctx->counts_pending = false;
        ctx->res_set = set;
        ctx->results_valid = true;
    }
    if (n_pass) *n_pass = ctx->n_pass;
    return PSK_OK;
}
