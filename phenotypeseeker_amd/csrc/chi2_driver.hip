// The chi2 scans' host side: what a scan launches with (fill_chi2_args, from the plan of chi2_plan.h), the launch itself and
// its repeats, and the exported calls.  No kernel lives here: the kernels are assoc_scan.hip's, reached through
// launch_chi2_any (chi2_launch.h), so an edit to this file leaves the hash of the kernels' source alone.
#include "chi2_launch.h"

#include <cmath>
#include <sched.h>

namespace {

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

// most workgroups of chi2_scan_kernel_cx_side: PSK_GRID_MULT per CU when set, else the kernel's own multiple
uint64_t cx_side_grid_cap(const psk_ctx *ctx) { return (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : PSK_CX_SIDE_GRID_MULT); }
// ... and of chi2_scan_kernel_cx_side_pc
uint64_t cx_pc_grid_cap(const psk_ctx *ctx) { return (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : PSK_CX_PC_GRID_MULT); }

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

// The arguments every form shares: the matrix, the masks, the cuts and the pre-test's threshold.
void fill_common_args(const psk_ctx *ctx, ScanArgs &a)
{
    const ScanParams &L = ctx->last;
    a = ScanArgs();
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
}

// The exception-coded path: the plan for this scan's key (kept in the context until the key changes), copied into the
// launch, and the result set bound to the plan's segment size.  The two knobs are read per scan: A/B runs and tests in
// one build.
int fill_cx_args(psk_ctx *ctx, Chi2Launch &CL, int set)
{
    CxScanArgs &x = CL.x;
    ScanArgs &a = x.s;
    int side_on = 1, pc_on = 1, idx_on = 1;
    PSK_TRY(env_choice(ctx, "PSK_CX_SIDE_KERNEL", {0, 1}, &side_on));
    PSK_TRY(env_choice(ctx, "PSK_CX_PC_FILTER", {0, 1}, &pc_on));
    PSK_TRY(env_choice(ctx, "PSK_CX_PC_INDEX", {0, 1}, &idx_on));
    CxPlanKey key;
    key.M = a.M; key.n_ov = ctx->cx_n_ov; key.cap = scan_grid_cap(ctx); key.side_cap = cx_side_grid_cap(ctx);
    key.pc_cap = cx_pc_grid_cap(ctx); key.pc_filter = pc_on; key.pc_index = idx_on;
    memcpy(&key.thr_bits, &a.cut.thr, 8);
    key.n1 = a.cut.n1; key.n0 = a.cut.n0; key.n_samples = ctx->n_samples; key.cpr = a.cpr;
    key.min_samples = a.cut.min_samples; key.max_samples = a.cut.max_samples; key.side_kernel = side_on;
    CxPlan &pl = ctx->cx_plan;
    if (!pl.valid || !(pl.key == key)) pl = cx_make_plan(key, ctx->cx_pc_hist.data(), ctx->cx_pc_hist.size());

    CL.form = pl.form;
    CL.cpr = a.cpr;
    CL.grid = dim3(pl.grid);
    x.slots = ctx->cx_slots.as<u32x4>();
    x.ov = ctx->cx_ov.as<u32x4>();
    x.ov_row = ctx->cx_ov_row.as<uint32_t>();
    x.n_ov = ctx->cx_n_ov;
    x.class_mask = pl.class_mask; x.corner[0] = pl.corner[0]; x.corner[1] = pl.corner[1];
    x.slot_blocks = pl.slot_blocks; x.ov_blocks = pl.ov_blocks;
    ctx->cx_last_plan = true;
    ctx->cx_last_filtered = pl.form == Chi2Form::CxSidePc || pl.form == Chi2Form::CxSideIdx;   // (which of the two: psk_last_scan_form)
    ctx->cx_last_rows_feasible = pl.rows_feasible;
    ctx->cx_last_class_mask = pl.class_mask;
    ctx->cx_last_skipped = pl.slot_blocks == 0;
    PSK_TRY(bind_results(ctx, a.sink, pl.seg_cap, set));
    if (pl.form != Chi2Form::CxMixed) {
        CxSideArgs &sd = CL.side.s;
        CL.side.ov_pc = ctx->cx_ov_pc.as<uint16_t>();
        memcpy(CL.side.feas, pl.feas, sizeof(CL.side.feas));
        sd.ov = x.ov; sd.ov_row = x.ov_row; sd.n_ov = x.n_ov;
        memcpy(sd.m1, a.m1_inl, sizeof(sd.m1));
        memcpy(sd.m0, a.m0_inl, sizeof(sd.m0));
        sd.cut = a.cut;
        sd.sink = a.sink;
        if (pl.form == Chi2Form::CxSideIdx) {
            CL.sidx.s = sd;
            CL.sidx.idx = ctx->cx_pc_index.as<uint32_t>();
            for (int r = 0; r < CX_IDX_RUNS; r++) { CL.sidx.run_begin[r] = (uint32_t)pl.runs.begin[r]; CL.sidx.run_len[r] = (uint32_t)pl.runs.len[r]; }
        }
    }
    return PSK_OK;
}

// The arguments of the last chi2 scan (ctx->last) for result set `set`.  Unit weights on a matrix with an exception-coded
// copy run over it, unless PSK_SCAN_DENSE=1 (read per call: A/B runs and tests in one build).
// build_tables: a new scan, whose weight table has just been uploaded (a repeated scan finds its table in place).
int fill_chi2_args(psk_ctx *ctx, Chi2Launch &CL, int set, bool build_tables)
{
    const ScanParams &L = ctx->last;
    ScanArgs &a = CL.x.s;
    ctx->last_form = -1;
    fill_common_args(ctx, a);
    ScanShape sh;   // weighted: class-weight sums from a table in LDS (e0 = class 1, e1 = class 0)
    PSK_TRY(setup_table_scan(ctx, a, L.weighted ? a.tab : nullptr, 2, L.W1, L.W0, 0.0, build_tables, &sh));
    ctx->cx_last_plan = false;
    if (ctx->cx_valid && !L.weighted && L.inline_masks && !env_flag("PSK_SCAN_DENSE")) {
        PSK_TRY(fill_cx_args(ctx, CL, set));
        ctx->last_form = (int)CL.form;
        return PSK_OK;
    }
    CL.form = Chi2Form::Dense;
    ctx->last_form = (int)CL.form;
    PSK_TRY(pick_chi2_mode(ctx, L.weighted, a.cut.pcut, a.cut.pcut_bonf, a.cut.omit_B, &CL.mode));
    CL.grid = sh.grid;
    return setup_results(ctx, a, CL.grid, group_lanes(a), sh.unroll, set, sh.threads);
}

// Launches the scan and returns without waiting; psk_scan_end collects it.  Lets a caller queue other work (the
// survivor exchange of the previous scan) while the kernel streams the matrix.
int chi2_scan_launch(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples, int max_samples,
                     double pvalue_cutoff, int omit_B, uint64_t n_kmers_global, bool keep_results)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->n_in_flight >= 2) return psk_fail(ctx, PSK_ESTATE, "two scans are in flight (psk_scan_end first)");
    if (!ctx->have_presence) return psk_fail(ctx, PSK_ESTATE, "no presence matrix (psk_build_presence first)");
    if (!pheno) return psk_fail(ctx, PSK_EINVAL, "null phenotype vector");
    if (n_kmers_global == 0) n_kmers_global = ctx->n_kmers ? ctx->n_kmers : 1;
    // How psk_scan_end learns that the scan is done (read per scan: A/B runs and tests in one build).  1: from the stamps
    // its kernel writes to pinned memory -- the dispatch carries no events; 0: from an event pair on the dispatch.  The
    // weighted scan is two kernels and keeps its events either way, and so do the scans of a context whose survivors are
    // exported on another stream (psk_export_survivors_async: that export needs the scan COMPLETE, not merely published).
    // A stamped scan of few enough workgroups (stamp_summary_used) is ended by the summary line its last publisher writes,
    // and its per-segment counts are read when a result call asks (PSK_SCAN_SUMMARY=1); 0: psk_scan_end waits for the 256
    // count words as well, sums them itself and keeps them -- the A/B switch of the host's side within one build (the
    // kernel writes the same words either way).  A larger launch writes no summary and is waited for word by word.
    int wait_by_stamps = 1, end_by_summary = 1;
    PSK_TRY(env_choice(ctx, "PSK_SCAN_WAIT", {0, 1}, &wait_by_stamps));
    PSK_TRY(env_choice(ctx, "PSK_SCAN_SUMMARY", {0, 1}, &end_by_summary));
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
        const bool stamped = wait_by_stamps == 1 && !weights && !ctx->exports_async;
        launch_chi2_any(ctx, CL, stamped ? TimedBy{} : TimedBy{sl.ev0, sl.ev1});   // (the events ride on the dispatch: one command per scan)
        PSK_HIP(ctx, hipGetLastError());
        sl.stamped = stamped;
        sl.has_summary = stamped && stamp_summary_used(CL.grid.x);   // (the kernel decides by the same function of its grid)
        sl.by_summary = sl.has_summary && end_by_summary == 1;
        sl.in_flight = true;
        ctx->n_in_flight++;
    } else {  // nothing to scan: an empty result, at once
        ctx->n_pass = 0;
        ctx->seg_counts.assign(SC_NSEG, 0);
        ctx->counts_pending = false;
        ctx->res_set = set;
        ctx->results_valid = true;
    }
    return PSK_OK;
}

int rescan(psk_ctx *ctx, int reps, double *mean_ms, double *ms_each)
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

}  // namespace

// Waits for words that the scan bound to result set `set` (launched without events) stamps into pinned memory: its summary
// line, which the scan's last publisher writes -- the scan has ended, n_pass and the clocks are there --, its count
// words, both, or -- a launch too large for the summary -- its count words and the clock beside each (StampWait,
// scan_common.h).  The host spins on pinned memory -- the words arrive while the kernel's last
// workgroups end --, asks the stream now and then whether the scan has failed or ended without a word, and gives up
// after WAIT_LIMIT: it never loops without a bound.  With clocks awaited, the scan's time is taken from them.
int wait_stamps(psk_ctx *ctx, int set, StampWait what)
{
    using clk = std::chrono::steady_clock;
    constexpr auto QUERY_EVERY = std::chrono::microseconds(20), YIELD_AFTER = std::chrono::microseconds(50);
    constexpr auto WAIT_LIMIT = std::chrono::seconds(30);
    const volatile uint64_t *words = scan_stamp_words(ctx, set);
    const uint32_t seq = (uint32_t)ctx->slot[set].seq;
    const bool want_summary = what == STAMP_WAIT_SUMMARY || what == STAMP_WAIT_ALL, want_counts = what != STAMP_WAIT_SUMMARY;
    int nc = want_counts ? 0 : STAMP_NSEG;   // count words seen so far: a stamp that has arrived stays
    int nk = what == STAMP_WAIT_SEGMENTS ? 0 : STAMP_CLOCKS;   // ... and clock words
    auto all_here = [&] {
        if (want_summary && !stamp_summary_ready(words, seq)) return false;
        if (nc < STAMP_NSEG) nc = stamp_counts_missing(words, seq, nc);
        if (nc == STAMP_NSEG && nk < STAMP_CLOCKS) nk = stamp_clocks_missing(words + STAMP_NSEG, seq, nk);
        return nc == STAMP_NSEG && nk == STAMP_CLOCKS;
    };
    if (!all_here()) {
        const clk::time_point t0 = clk::now();
        clk::time_point next_query = t0 + QUERY_EVERY;
        for (;;) {
            __builtin_ia32_pause();
            if (all_here()) break;
            const clk::time_point now = clk::now();
            if (now >= next_query) {
                const hipError_t e = hipStreamQuery(ctx->stream);
                if (e == hipSuccess) {   // everything queued has ended: the words are there now, or never will be
                    if (all_here()) break;
                    if (want_summary && !stamp_summary_ready(words, seq)) return psk_fail(ctx, PSK_ESTATE, "scan ended without publishing (summary of scan %u)", seq);
                    return psk_fail(ctx, PSK_ESTATE, "scan ended without publishing (segment %d of scan %u)", nc < STAMP_NSEG ? nc : nk, seq);
                }
                if (e != hipErrorNotReady) return psk_fail(ctx, PSK_EHIP, "hipStreamQuery failed while scan %u was awaited: %s", seq, hipGetErrorString(e));
                (void)hipGetLastError();   // "not ready" is an answer, not an error for the next launch's check to find
                if (now - t0 > WAIT_LIMIT) return psk_fail(ctx, PSK_ESTATE, "scan %u has not published its counts after 30 s", seq);
                next_query = clk::now() + QUERY_EVERY;
            }
            if (now - t0 > YIELD_AFTER) sched_yield();
        }
    }
    if (want_summary) ctx->last_scan_ms = (double)stamp_summary_ticks(words) / ctx->wall_clock_khz;
    if (what == STAMP_WAIT_SEGMENTS) ctx->last_scan_ms = (double)stamp_scan_ticks(words + STAMP_NSEG) / ctx->wall_clock_khz;
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
        bool counts_later = false;
        if (sl.stamped) {
            // the kernel's own words: no event on the dispatch, no runtime call when the GPU is ahead
            const int rc = wait_stamps(ctx, set, sl.by_summary ? STAMP_WAIT_SUMMARY : sl.has_summary ? STAMP_WAIT_ALL : STAMP_WAIT_SEGMENTS);
            sl.in_flight = false;
            ctx->n_in_flight--;
            PSK_TRY(rc);
            if (sl.by_summary) {
                // one line says it all: n_pass, and whether a segment overflowed.  Only then are the count words waited
                // for and read here, so that PSK_ERANGE comes from this call as it always has (fetch_counts).
                const volatile uint64_t *words = scan_stamp_words(ctx, set);
                const uint64_t hi = stamp_load(words + STAMP_SUM_HI);
                if (stamp_sum_overflow(hi)) PSK_TRY(wait_stamps(ctx, set, STAMP_WAIT_COUNTS));
                else {
                    hold_results_unread(ctx, set, stamp_sum_n_pass(stamp_load(words + STAMP_SUM_LO), hi));
                    counts_later = true;
                }
            }
        } else {
            PSK_HIP(ctx, hipEventSynchronize(sl.ev1));  // its kernels have written the counts to pinned memory
            sl.in_flight = false;
            ctx->n_in_flight--;
            float ms = 0;
            PSK_HIP(ctx, hipEventElapsedTime(&ms, sl.ev0, sl.ev1));
            ctx->last_scan_ms = ms;
        }
        if (!counts_later) PSK_TRY(fetch_counts(ctx, set));
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
    cx_plan(plan_cuts(n1, n0, min_samples, max_samples, thr), n_samples, class_mask, corner);
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
    cx_pc_plan(plan_cuts(n1, n0, min_samples, max_samples, thr), n_samples, feas);
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

extern "C" int psk_cx_idx_plan(const uint64_t *feas, const uint64_t *pc_hist, int n_hist, uint64_t n_ov, int knob_on, uint64_t *begin,
                               uint64_t *len, int *n_runs, uint64_t *rows, int *chosen)
{
    if (!feas || !pc_hist || n_hist < 0 || !begin || !len || !n_runs) return PSK_EINVAL;
    const cx_idx_runs_t r = cx_idx_runs(feas, pc_hist, (size_t)n_hist);
    for (int i = 0; i < CX_IDX_RUNS; i++) { begin[i] = r.begin[i]; len[i] = r.len[i]; }
    *n_runs = r.n;
    if (rows) *rows = r.rows;
    if (chosen) *chosen = cx_idx_chosen(r, n_ov, knob_on) ? 1 : 0;
    return PSK_OK;
}

extern "C" int psk_cx_idx_shape(uint64_t n_rows, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block, uint32_t *threads,
                                uint64_t *seg_cap)
{
    if (cap_blocks < 1 || cap_blocks > 0xffffffffull || !blocks || !rows_per_block) return PSK_EINVAL;
    const cx_side_shape_t sh = cx_idx_shape(n_rows, cap_blocks);
    *blocks = sh.blocks;
    *rows_per_block = sh.rows_per_block;
    if (threads) *threads = sh.batch_rows;
    if (seg_cap) *seg_cap = result_seg_cap((uint64_t)sh.blocks, sh.rows_per_block);
    return PSK_OK;
}

extern "C" int psk_last_scan_form(const psk_ctx *ctx, int *form)
{
    if (!ctx || !form) return PSK_EINVAL;
    *form = ctx->last_form;
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
