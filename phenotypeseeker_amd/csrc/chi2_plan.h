// Everything the host decides about a chi2 scan, as plain arithmetic: the candidate rule the kernels share with the plans,
// what a scan's parameters leave of the exception-coded rows (cx_plan, cx_pc_plan), the launch shapes of the three
// exception-coded kernels, the size of a result segment, and the plan that is kept from scan to scan (cx_make_plan).
// Nothing here touches the device, a context or the environment (knob values arrive in the key), so it can be read,
// compiled and checked on its own: tests/cx_plan_check.cpp.  The kernels are assoc_scan.hip's, the driver chi2_driver.hip.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// what host and device evaluate alike: -ffp-contract=off on both sides, so the same IEEE double operations
#ifdef __HIPCC__
#define CHI2_SHARED __host__ __device__ inline __attribute__((always_inline))   // = __forceinline__, which only the HIP runtime header defines
#else
#define CHI2_SHARED inline
#endif

// What decides a row: the class sizes (popcounts of the masks), the frequency filter and the cut-offs.
struct ScanCuts {
    double pcut, pcut_bonf, thr;  // thr: statistic threshold of the division-free pre-test
    int n1, n0;
    int min_samples, max_samples;
    int omit_B;
};

// the division-free pre-test of a unit-weight 2 x 2 table: chi2 = T (AD - BC)^2 / (R1 R0 K1 K0) cannot be ruled out
// against thr.  Host and device evaluate it in the same IEEE double operations: the host's corner table of the
// exception-coded scan (cx_plan) decides bit for bit what the dense kernel decides.
CHI2_SHARED bool chi2_pretest(double A, double B, double C, double D, double thr)
{
    const double R1 = A + B, R0 = C + D, K1 = A + C, K0 = B + D, T = R1 + R0;
    const double det = A * D - B * C;
    const double lhs = T * det * det, rhs = thr * R1 * R0 * K1 * K0;
    return !(lhs < rhs * (1.0 - 1e-9));  // NaN compares false -> a candidate
}

// The frequency filter on a row's two class counts (the weighted scan queues on it alone).  A kernel's lane adds its own
// condition where it has always stood in the chain: `exists`, the row index is inside the matrix.
CHI2_SHARED bool chi2_freq_ok(const ScanCuts &K, uint32_t a, uint32_t c, bool exists = true)
{
    const int n_w = (int)(a + c);
    const int n_wo = (K.n1 - (int)a) + (K.n0 - (int)c);
    return exists && !(n_w < K.min_samples || n_wo < 2 || n_w > K.max_samples);
}

// THE CANDIDATE RULE of a unit-weight row with a case and c control samples: it passes the filter and the pre-test cannot
// rule it out.  The dense kernel (MODE 0 and 2) and both plans below decide through this one function; the side-row code
// of the exception-coded kernels restates the same operations by hand (its register counts changed through the call;
// assoc_scan.hip, SideRows), so there the agreement is kept by the GPU tests, not by structure.  The scan's exactness is
// that all of them agree bit for bit.  `answers`, a lane's second condition (of the lanes that share the row, this one
// reports it), stands before the pre-test as it always has.
CHI2_SHARED bool chi2_candidate(const ScanCuts &K, uint32_t a, uint32_t c, bool exists = true, bool answers = true)
{
    const bool freq_ok = chi2_freq_ok(K, a, c, exists);
    const double A = (double)a, B = (double)(K.n1 - (int)a), C = (double)c, D = (double)(K.n0 - (int)c);
    return freq_ok && answers && chi2_pretest(A, B, C, D, K.thr);
}

// the cuts a plan depends on (the p cut-offs decide only after the exact statistic)
inline ScanCuts plan_cuts(int n1, int n0, int min_samples, int max_samples, double thr)
{
    ScanCuts K = {};
    K.thr = thr;
    K.n1 = n1; K.n0 = n0;
    K.min_samples = min_samples; K.max_samples = max_samples;
    return K;
}

// ---- what a scan's parameters leave of the exception-coded rows ------------------------------------------------------
constexpr int CX_MAX_E = 7;   // exceptions a slot holds (presence_compact.hip); rows with more are the side matrix

// What a scan's parameters leave of the slot rows.  corner[base] bit a' * 8 + c' (a', c' <= 7): the table of a slot row
// with a' case and c' control exceptions -- (a', c') when the exceptions are the present samples (base 0), (n1 - a',
// n0 - c') when they are the absent ones (base 1) -- is a candidate; 0 where a' > n1 or c' > n0: no row has such a table.
// class_mask bit (e | base << 3): a row of e exceptions can have a table whose bit is set.  Its a' + c' is e less its
// exceptions among the NA samples, of which there are n_samples - n1 - n0.  (n1 = 0, n0 = 0: the pre-test lets every NaN
// table through, the filter alone decides.)
inline void cx_plan(const ScanCuts &K, int n_samples, uint32_t *class_mask, uint64_t corner[2])
{
    corner[0] = corner[1] = 0;
    for (int base = 0; base < 2; base++)
        for (int ap = 0; ap <= CX_MAX_E && ap <= K.n1; ap++)
            for (int cp = 0; cp <= CX_MAX_E && cp <= K.n0; cp++)
                if (chi2_candidate(K, (uint32_t)(base ? K.n1 - ap : ap), (uint32_t)(base ? K.n0 - cp : cp))) corner[base] |= 1ull << (ap * 8 + cp);
    const int n_na = n_samples - K.n1 - K.n0;
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
// doubles.)  Two candidate tests per s, n1 + n0 + 1 values of s.
inline void cx_pc_plan(const ScanCuts &K, int n_samples, uint64_t feas[4])
{
    const int T = K.n1 + K.n0, n_na = n_samples - T;
    std::vector<int> ok_upto(T + 2, 0);   // ok_upto[s + 1]: sums <= s that pass
    for (int s = 0; s <= T; s++) {
        const int ends[2] = {std::max(0, s - K.n0), std::min(s, K.n1)};
        const bool ok = chi2_candidate(K, (uint32_t)ends[0], (uint32_t)(s - ends[0])) || chi2_candidate(K, (uint32_t)ends[1], (uint32_t)(s - ends[1]));
        ok_upto[s + 1] = ok_upto[s] + (ok ? 1 : 0);
    }
    feas[0] = feas[1] = feas[2] = feas[3] = 0;
    for (int pc = 0; pc < 256; pc++) {
        const int lo = std::max(0, pc - n_na), hi = std::min(pc, T);
        if (lo <= hi && ok_upto[hi + 1] - ok_upto[lo] > 0) feas[pc >> 6] |= 1ull << (pc & 63);
    }
}

// ---- launch shapes ----------------------------------------------------------------------------------------------------
// The constants the shapes share with the kernels (overridable at build time for A/B runs: make EXTRA=-DPSK_CX_...=...)
#ifndef PSK_CX_UNROLL
#define PSK_CX_UNROLL 4
#endif
#ifndef PSK_CX_SIDE_UNROLL
#define PSK_CX_SIDE_UNROLL 2
#endif
#ifndef PSK_CX_PC_UNROLL
#define PSK_CX_PC_UNROLL 8
#endif
#ifndef PSK_CX_SIDE_GRID_MULT
#define PSK_CX_SIDE_GRID_MULT 8   // workgroups per CU of chi2_scan_kernel_cx_side when PSK_GRID_MULT is unset (r13 table: 8 before 4 and the one-batch grid)
#endif
#ifndef PSK_CX_PC_GRID_MULT
#define PSK_CX_PC_GRID_MULT 8   // ... of chi2_scan_kernel_cx_side_pc
#endif
constexpr int CX_UNROLL = PSK_CX_UNROLL;             // chi2_scan_kernel_cx: 16-byte loads in flight per lane
constexpr int CX_SIDE_UNROLL = PSK_CX_SIDE_UNROLL;   // ..._cx_side: 16-byte loads in flight per lane and register set
constexpr int CX_PC_UNROLL = PSK_CX_PC_UNROLL;       // ..._cx_side_pc: 2-byte loads in flight per lane and register set
static_assert(CX_PC_UNROLL == 4 || CX_PC_UNROLL == 8, "a batch is 256 or 512 rows");
#ifndef PSK_CX_IDX_THREADS
#define PSK_CX_IDX_THREADS 64   // threads per workgroup of chi2_scan_kernel_cx_side_idx (r25 table: 64 against 256)
#endif
#ifndef PSK_CX_IDX_SHARE
#define PSK_CX_IDX_SHARE 8      // the index form runs when rows_feasible * CX_IDX_SHARE <= n_ov (r25 table)
#endif
constexpr int CX_IDX_THREADS = PSK_CX_IDX_THREADS;   // ..._cx_side_idx: one feasible row per lane and pass
static_assert(CX_IDX_THREADS == 64 || CX_IDX_THREADS == 256, "whole waves, at most a scan workgroup");
constexpr uint64_t CX_IDX_SHARE = PSK_CX_IDX_SHARE;
constexpr int CX_IDX_RUNS = 4;                       // index ranges the kernel's arguments hold
constexpr int CX_WAVES = 4;                          // waves per workgroup (SC_THREADS / 64)
constexpr int CX_NSEG = 256;                         // SC_NSEG: every result segment needs a workgroup to publish its count

// entries per result segment: what the workgroups of one segment (segment = blockIdx % CX_NSEG) can visit
inline uint64_t result_seg_cap(uint64_t blocks, uint64_t rows_per_block)
{
    const uint64_t blocks_per_seg = (blocks + CX_NSEG - 1) / CX_NSEG;
    const uint64_t seg_cap = blocks_per_seg * rows_per_block;
    return seg_cap < 64 ? 64 : seg_cap;
}

struct cx_side_shape_t {
    uint32_t blocks;          // workgroups of the launch
    uint64_t rows_per_block;  // the most rows one of them visits
    uint32_t batch_rows;      // rows of one wave batch
};

// chi2_scan_kernel_cx_side's sweep: a row of the side matrix is cpr 16-byte chunks, one lane each, so a wave step covers
// 64 / cpr rows and a batch -- what a wave loads before it evaluates -- CX_SIDE_UNROLL steps.  Wave w of the launch's W
// waves takes the batches w, w + W, w + 2 W, ... (grid-stride), and W = blocks * CX_WAVES: every workgroup sweeps.
// cap_blocks: the most workgroups the launch may have (CUs x the grid multiple).  blocks = what one batch per wave would
// need, capped, and never below CX_NSEG; rows_per_block bounds the rows of the waves' batches, full or not.
inline cx_side_shape_t cx_side_shape(uint64_t n_ov, int cpr, uint64_t cap_blocks)
{
    const uint64_t rpw = 64 / (uint64_t)cpr;
    const uint64_t steps = (n_ov + rpw - 1) / rpw;
    const uint64_t batches = (steps + CX_SIDE_UNROLL - 1) / CX_SIDE_UNROLL;
    uint64_t blocks = (batches + CX_WAVES - 1) / CX_WAVES;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < CX_NSEG) blocks = CX_NSEG;
    const uint64_t waves = blocks * CX_WAVES;
    const uint64_t passes = (batches + waves - 1) / waves;   // batches of wave 0, the most any wave takes
    cx_side_shape_t s;
    s.blocks = (uint32_t)blocks;
    s.batch_rows = (uint32_t)(CX_SIDE_UNROLL * rpw);
    s.rows_per_block = passes * CX_WAVES * s.batch_rows;
    return s;
}

// The popcount-filtered sweep (chi2_scan_kernel_cx_side_pc): a row is one lane, a wave step 64 rows and a batch
// CX_PC_UNROLL steps -- the 2-byte popcounts a wave loads before it looks at any row.  Batches are dealt to the waves
// grid-stride exactly as above.
inline cx_side_shape_t cx_pc_shape(uint64_t n_ov, uint64_t cap_blocks)
{
    const uint64_t batch_rows = 64 * (uint64_t)CX_PC_UNROLL;
    const uint64_t batches = (n_ov + batch_rows - 1) / batch_rows;
    uint64_t blocks = (batches + CX_WAVES - 1) / CX_WAVES;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < CX_NSEG) blocks = CX_NSEG;
    const uint64_t waves = blocks * CX_WAVES;
    const uint64_t passes = (batches + waves - 1) / waves;   // batches of wave 0, the most any wave takes
    cx_side_shape_t s;
    s.blocks = (uint32_t)blocks;
    s.batch_rows = (uint32_t)batch_rows;
    s.rows_per_block = passes * CX_WAVES * batch_rows;
    return s;
}

// The indexed sweep (chi2_scan_kernel_cx_side_idx): T rows -- the feasible ones, found through the encoder's index of
// the side matrix by popcount -- one per lane, workgroup b taking rows (p * blocks + b) * CX_IDX_THREADS + thread of pass
// p.  As many workgroups as the rows need and no more: NOT raised to CX_NSEG, the segments beyond the grid are
// published by workgroup 0 (publish_unowned_segments, scan_common.h).  T = 0: one workgroup, which only publishes.
inline cx_side_shape_t cx_idx_shape(uint64_t T, uint64_t cap_blocks)
{
    uint64_t blocks = (T + CX_IDX_THREADS - 1) / CX_IDX_THREADS;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < 1) blocks = 1;
    const uint64_t per_pass = blocks * CX_IDX_THREADS;
    const uint64_t passes = (T + per_pass - 1) / per_pass;
    cx_side_shape_t s;
    s.blocks = (uint32_t)blocks;
    s.batch_rows = (uint32_t)CX_IDX_THREADS;
    s.rows_per_block = passes * CX_IDX_THREADS;
    return s;
}

// Where the feasible rows lie in the encoder's index (cx_pc_index: the side-matrix rows grouped by popcount, bucket pc
// starting at the exclusive prefix of the histogram): the feasible, non-empty buckets as ranges [begin, begin + len) of
// index positions.  Buckets that follow each other in the index are one range -- adjacent feasible buckets, and feasible
// buckets with only empty ones between them.  n: all ranges there are; the first CX_IDX_RUNS of them are kept (a plan
// with more is not an index plan).  rows: what they hold, the plan's rows_feasible.
struct cx_idx_runs_t {
    int n = 0;
    uint64_t rows = 0;
    uint64_t begin[CX_IDX_RUNS] = {0, 0, 0, 0}, len[CX_IDX_RUNS] = {0, 0, 0, 0};
};
inline cx_idx_runs_t cx_idx_runs(const uint64_t feas[4], const uint64_t *pc_hist, size_t n_hist)
{
    cx_idx_runs_t r;
    uint64_t pos = 0, end = 0;   // start of bucket pc; end of the last range
    for (size_t pc = 0; pc < n_hist; pc++) {
        const uint64_t h = pc_hist[pc];
        if (h && pc < 256 && ((feas[pc >> 6] >> (pc & 63)) & 1ull)) {
            if (r.n > 0 && end == pos) {
                if (r.n <= CX_IDX_RUNS) r.len[r.n - 1] += h;
            } else {
                if (r.n < CX_IDX_RUNS) { r.begin[r.n] = pos; r.len[r.n] = h; }
                r.n++;
            }
            end = pos + h;
            r.rows += h;
        }
        pos += h;
    }
    return r;
}

// the index form is worth its launch: few ranges, and few rows against what the popcount filter would read past
inline bool cx_idx_chosen(const cx_idx_runs_t &r, uint64_t n_ov, int knob_on)
{
    return knob_on && r.n <= CX_IDX_RUNS && r.rows * CX_IDX_SHARE <= n_ov;
}

struct cx_mixed_shape_t {
    uint32_t slot_blocks;     // workgroups [0, slot_blocks) stream the slots (none when no class is feasible),
    uint32_t ov_blocks;       // the next ov_blocks the side matrix; any beyond only publish their segment
    uint32_t blocks;          // workgroups of the launch
    uint64_t rows_per_block;  // the most rows one of them visits
};

// The mixed kernel (chi2_scan_kernel_cx): a lane's 16-byte load is a pair of slots, a wave batch CX_UNROLL x 64 pairs or
// CX_UNROLL steps of 64 / cpr side-matrix rows.  Workgroups of the two parts in proportion to their bytes, under `cap`
// (scan_grid_cap); with no feasible class (!any_class) the slots get none and the side matrix the whole cap.  At least
// CX_NSEG workgroups.
inline cx_mixed_shape_t cx_mixed_shape(uint64_t M, uint64_t n_ov, int cpr, uint64_t cap, bool any_class)
{
    const uint64_t wpb = CX_WAVES;
    const uint64_t n_pairs = (M + 1) / 2, ov_rpw = 64 / (uint64_t)cpr;
    // (at least one slot workgroup with a feasible class, so that slot_blocks == 0 says "no class" for every M: only M = 0,
    // which is never encoded, would give none)
    uint64_t bs = any_class ? std::max<uint64_t>(((n_pairs + 64 * CX_UNROLL - 1) / (64 * CX_UNROLL) + wpb - 1) / wpb, 1) : 0;
    uint64_t bo = (((n_ov + ov_rpw - 1) / ov_rpw + CX_UNROLL - 1) / CX_UNROLL + wpb - 1) / wpb;
    if (!any_class) bo = std::min(bo, cap);
    else if (bs + bo > cap) {
        const double slot_bytes = 16.0 * n_pairs, ov_bytes = 16.0 * cpr * n_ov;
        const uint64_t s = (uint64_t)(cap * slot_bytes / (slot_bytes + ov_bytes) + 0.5);
        bs = std::min(bs, std::max<uint64_t>(s, 1));
        bo = std::min(bo, cap - bs);
        if (n_ov && bo == 0) { bo = 1; bs = std::max<uint64_t>(bs - 1, 1); }
    }
    uint64_t total = bs + bo;
    if (total < CX_NSEG) {
        if (any_class) bs = CX_NSEG - bo;   // (more slot workgroups than slot work: they find p0 >= n_pairs)
        total = CX_NSEG;
    }
    const uint64_t ws = bs * wpb, wo = bo * wpb;
    const uint64_t cs = (n_pairs + 64 - 1) / 64, co = (n_ov + ov_rpw - 1) / ov_rpw;   // wave steps
    const uint64_t rs = ws ? (cs + ws * CX_UNROLL - 1) / (ws * CX_UNROLL) * wpb * CX_UNROLL * 128 : 0;
    const uint64_t ro = wo ? (co + wo * CX_UNROLL - 1) / (wo * CX_UNROLL) * wpb * CX_UNROLL * ov_rpw : 0;
    cx_mixed_shape_t s;
    s.slot_blocks = (uint32_t)bs;
    s.ov_blocks = (uint32_t)bo;
    s.blocks = (uint32_t)total;
    s.rows_per_block = std::max(rs, ro);
    return s;
}

// ---- the plan of an exception-coded scan, kept from scan to scan ------------------------------------------------------
// The five kernel forms of a chi2 scan: the dense kernels (chi2_scan_kernel and, weighted, its finalize pass), and over
// the exception-coded copy the mixed kernel, the side matrix alone, the side matrix through its popcounts, and the
// feasible rows of the side matrix through the encoder's index by popcount.  (psk_last_scan_form reports the value.)
enum class Chi2Form { Dense, CxMixed, CxSide, CxSidePc, CxSideIdx };

// Everything a plan is a function of -- none of it derived from WHICH samples are cases.  A scan with another key
// recomputes; a new matrix or encoded copy drops the plan.  (cpr follows from n_samples: it is here as an input.)
struct CxPlanKey {
    uint64_t M = 0, n_ov = 0, cap = 0, side_cap = 0, pc_cap = 0, thr_bits = 0;
    int n1 = 0, n0 = 0, n_samples = 0, cpr = 0, min_samples = 0, max_samples = 0, side_kernel = 0, pc_filter = 0, pc_index = 0;
    bool operator==(const CxPlanKey &o) const
    {
        return M == o.M && n_ov == o.n_ov && cap == o.cap && side_cap == o.side_cap && pc_cap == o.pc_cap && thr_bits == o.thr_bits &&
               n1 == o.n1 && n0 == o.n0 && n_samples == o.n_samples && cpr == o.cpr && min_samples == o.min_samples &&
               max_samples == o.max_samples && side_kernel == o.side_kernel && pc_filter == o.pc_filter && pc_index == o.pc_index;
    }
};
struct CxPlan {
    bool valid = false;
    CxPlanKey key;
    uint32_t class_mask = 0;
    uint64_t corner[2] = {0, 0};
    Chi2Form form = Chi2Form::CxMixed;
    uint32_t grid = 0, slot_blocks = 0, ov_blocks = 0;   // the side forms: slot_blocks = 0, ov_blocks = grid
    uint64_t seg_cap = 0;            // entries per result segment
    // the popcounts a side-matrix row must have for some table of it to be a candidate (cx_pc_plan), and how many rows
    // have one (the encoder's histogram)
    uint64_t feas[4] = {0, 0, 0, 0};
    uint64_t rows_feasible = 0;
    cx_idx_runs_t runs;              // CxSideIdx: where those rows lie in the index (cx_idx_runs)
};

// The plan for `key`.  The side matrix alone (CxSide) when the knob allows it and no header class is feasible; through its
// popcounts (CxSidePc) when, in addition, the filter knob is on and the histogram (pc_hist[pc], pc < n_hist: side-matrix
// rows of that popcount) says fewer than all rows can pass; of those plans, through the index (CxSideIdx) when the index
// knob is on and the feasible rows are few and lie in few ranges (cx_idx_chosen); else the mixed kernel.
inline CxPlan cx_make_plan(const CxPlanKey &key, const uint64_t *pc_hist, size_t n_hist)
{
    CxPlan pl;
    double thr;
    memcpy(&thr, &key.thr_bits, 8);
    const ScanCuts K = plan_cuts(key.n1, key.n0, key.min_samples, key.max_samples, thr);
    cx_plan(K, key.n_samples, &pl.class_mask, pl.corner);
    pl.form = key.side_kernel && pl.class_mask == 0 ? Chi2Form::CxSide : Chi2Form::CxMixed;
    pl.rows_feasible = key.n_ov;
    pl.feas[0] = pl.feas[1] = pl.feas[2] = pl.feas[3] = ~0ull;
    if (pl.form == Chi2Form::CxSide && key.pc_filter) {
        cx_pc_plan(K, key.n_samples, pl.feas);
        pl.rows_feasible = 0;
        for (size_t pc = 0; pc < n_hist && pc < 256; pc++)
            if ((pl.feas[pc >> 6] >> (pc & 63)) & 1ull) pl.rows_feasible += pc_hist[pc];
        bool filtered = pl.rows_feasible < key.n_ov;
#ifdef PSK_CX_PC_FORCE   // A/B builds: the filtered form whatever the count (the all-feasible comparison of the r15 table)
        filtered = true;
#endif
        if (filtered) pl.form = Chi2Form::CxSidePc;
        if (filtered && key.pc_index) {
            const cx_idx_runs_t r = cx_idx_runs(pl.feas, pc_hist, n_hist);
            if (cx_idx_chosen(r, key.n_ov, key.pc_index)) { pl.form = Chi2Form::CxSideIdx; pl.runs = r; }
        }
    }
    uint64_t rows_per_block;
    if (pl.form == Chi2Form::CxMixed) {
        const cx_mixed_shape_t sh = cx_mixed_shape(key.M, key.n_ov, key.cpr, key.cap, pl.class_mask != 0);
        pl.grid = sh.blocks; pl.slot_blocks = sh.slot_blocks; pl.ov_blocks = sh.ov_blocks;
        rows_per_block = sh.rows_per_block;
    } else {
        const cx_side_shape_t sh = pl.form == Chi2Form::CxSideIdx ? cx_idx_shape(pl.runs.rows, key.pc_cap)
                                   : pl.form == Chi2Form::CxSidePc ? cx_pc_shape(key.n_ov, key.pc_cap) : cx_side_shape(key.n_ov, key.cpr, key.side_cap);
        pl.grid = sh.blocks; pl.slot_blocks = 0; pl.ov_blocks = sh.blocks;
        rows_per_block = sh.rows_per_block;
    }
    pl.seg_cap = result_seg_cap(pl.grid, rows_per_block);
    pl.key = key;
    pl.valid = true;
    return pl;
}
