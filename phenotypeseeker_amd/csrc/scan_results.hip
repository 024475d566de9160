// The result sets of the association scans (chi2_driver.hip, ttest_scan.hip): the launch shape and the segmented result
// arrays that follow from it, the per-segment counts, and the calls that hand the survivors out.
#include "scan_common.h"

#include <algorithm>
#include <numeric>

// u64 words of a phenotype mask / 64-sample blocks of a per-sample table: the row's words rounded up to a whole chunk
int mask_words(const psk_ctx *ctx) { return (ctx->wpr + 1) & ~1; }

// lanes that own one row; 0 = half a lane (8-byte rows: chi2_scan_kernel's G = 0)
int group_lanes(const ScanArgs &a)
{
    if (a.half) return 0;
    int G = 1;
    while (G < a.cpr && G < 64) G <<= 1;
    return G;
}

// result arrays (SoA) inside ctx->res: row u64 | stat f64 | p f64 | mx f64 | my f64 | nw i32, each
// SC_NSEG * seg_cap entries; seg_cap bounds the rows the blocks of one segment can visit
// (rows_per_block: the most rows one workgroup of the launch visits)
uint64_t result_seg_cap(dim3 grid, uint64_t rows_per_block) { return result_seg_cap((uint64_t)grid.x, rows_per_block); }

// Result set `set` with segments of seg_cap entries, as a kernel addresses it.  The layout is worked out when the set's
// buffer is reserved or seg_cap changes (the buffer only ever grows, and only here); a scan of the same shape copies it.
int bind_results(psk_ctx *ctx, ScanSink &s, uint64_t seg_cap, int set)
{
    if (seg_cap >= (1ull << 32)) return psk_fail(ctx, PSK_ERANGE, "result segment too large");
    ScanSlot &sl = ctx->slot[set];
    if (!sl.sink_valid || sl.sink.seg_cap != (uint32_t)seg_cap) {
        sl.sink_valid = false;
        const uint64_t cap = seg_cap * SC_NSEG;
        DevBuf &rb = sl.res;
        PSK_TRY(dev_reserve(ctx, rb, cap * 44 + 64));
        uint8_t *b = rb.as<uint8_t>();
        ScanSink &a = sl.sink;
        a.res_row = reinterpret_cast<uint64_t *>(b);
        a.res_stat = reinterpret_cast<double *>(b + cap * 8);
        a.res_p = reinterpret_cast<double *>(b + cap * 16);
        a.res_mx = reinterpret_cast<double *>(b + cap * 24);
        a.res_my = reinterpret_cast<double *>(b + cap * 32);
        a.res_nw = reinterpret_cast<int32_t *>(b + cap * 40);
        if (!ctx->res_count.p) {  // counters (the ticket line among them) re-arm themselves at the end of every scan: zeroed once
            PSK_TRY(dev_reserve(ctx, ctx->res_count, SC_COUNTER_WORDS * 4));
            PSK_HIP(ctx, hipMemsetAsync(ctx->res_count.p, 0, SC_COUNTER_WORDS * 4, ctx->stream));
        }
        if (!ctx->cnt_pinned) {
            // coherent, said explicitly: the host reads the stamps while the kernel that writes them still runs.  Zeroed:
            // launch numbers start at 1, so a word no scan has written carries no scan's tag.
            void *blk = nullptr, *hc = nullptr;
            PSK_HIP(ctx, hipHostMalloc(&blk, 2 * STAMP_SET_WORDS * 8, hipHostMallocCoherent));
            memset(blk, 0, 2 * STAMP_SET_WORDS * 8);
            if (hipHostGetDevicePointer(&hc, blk, 0) != hipSuccess) {
                (void)hipHostFree(blk);
                return psk_fail(ctx, PSK_EHIP, "hipHostGetDevicePointer failed for the scans' stamp block");
            }
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) {
                (void)hipHostFree(blk);
                return psk_fail(ctx, PSK_EHIP, "the device reports no wall clock rate");
            }
            ctx->wall_clock_khz = khz;
            ctx->cnt_pinned = blk;
            ctx->cnt_pinned_dev = static_cast<uint64_t *>(hc);
        }
        a.counter = ctx->res_count.as<uint32_t>();
        a.final_counts = a.counter + SC_NSEG * SC_CNT_STRIDE + set * SC_NSEG;  // one compact array per result set
        a.host_counts = ctx->cnt_pinned_dev + set * STAMP_SET_WORDS;
        a.seg_cap = (uint32_t)seg_cap;
        sl.sink_valid = true;
    }
    sl.stamped = false;         // (chi2_scan_launch says otherwise after it has launched without events)
    sl.seq = ctx->scan_seq++;   // the scan being set up: its place in the launch order and the tag of its stamps
    s = sl.sink;
    s.seq = (uint32_t)sl.seq;
    sl.seg_cap = seg_cap;
    if (set == ctx->res_set) {  // the last ended scan's results are about to go, its count words with them, read or not
        ctx->results_valid = false;
        ctx->counts_pending = false;
    }
    return PSK_OK;
}

// the stamp words of result set `set` as the host reads them: STAMP_NSEG counts, then STAMP_CLOCKS clocks
const volatile uint64_t *scan_stamp_words(const psk_ctx *ctx, int set)
{
    return static_cast<const volatile uint64_t *>(ctx->cnt_pinned) + set * STAMP_SET_WORDS;
}

int setup_results_rows(psk_ctx *ctx, ScanSink &s, dim3 grid, uint64_t rows_per_block, int set)
{
    return bind_results(ctx, s, result_seg_cap(grid, rows_per_block), set);
}

int setup_results(psk_ctx *ctx, ScanArgs &a, dim3 grid, int G, int unroll, int set, int threads)
{
    const uint64_t rpw = sc_rpw(G);
    const uint64_t n_steps = (a.M + rpw - 1) / rpw;
    const uint64_t total_waves = (uint64_t)grid.x * (threads / 64);
    const uint64_t iters = (n_steps + total_waves * unroll - 1) / (total_waves * unroll);
    return setup_results_rows(ctx, a.sink, grid, (threads / 64) * iters * unroll * rpw, set);
}

// per-segment counts of the scan that wrote result set `set`, as its kernels left them in pinned host memory (after
// that scan has been waited for, by event or by these very stamps); n_pass = their sum.  The set becomes the one the
// result calls read.  Every word must carry the scan's launch number: a count of another scan is never handed out.
int fetch_counts(psk_ctx *ctx, int set)
{
    const volatile uint64_t *raw = scan_stamp_words(ctx, set);
    const uint64_t seg_cap = ctx->slot[set].seg_cap;
    const uint32_t seq = (uint32_t)ctx->slot[set].seq;
    ctx->seg_counts.assign(SC_NSEG, 0);
    uint64_t tot = 0;
    for (int s = 0; s < SC_NSEG; s++) {
        const uint64_t w = stamp_load(raw + s);
        if (stamp_word_seq(w) != seq)
            return psk_fail(ctx, PSK_ESTATE, "result segment %d carries the count of scan %u, not of scan %u", s, stamp_word_seq(w), seq);
        const uint32_t c = stamp_word_count(w);
        if (c > seg_cap) return psk_fail(ctx, PSK_ERANGE, "result segment %d overflowed (%u > %llu)", s, c, (unsigned long long)seg_cap);
        ctx->seg_counts[s] = c;
        tot += c;
    }
    ctx->n_pass = tot;
    ctx->res_set = set;
    ctx->res_seg_cap = seg_cap;
    ctx->results_valid = true;
    ctx->counts_pending = false;
    return PSK_OK;
}

// What psk_scan_end leaves of a scan it ended by the summary line alone (chi2_driver.hip): n_pass and the set, with the
// per-segment counts still where the kernel wrote them.
void hold_results_unread(psk_ctx *ctx, int set, uint64_t n_pass)
{
    ctx->n_pass = n_pass;
    ctx->res_set = set;
    ctx->res_seg_cap = ctx->slot[set].seg_cap;
    ctx->results_valid = true;
    ctx->counts_pending = true;
}

// The one way to the per-segment counts of the held results (the caller has checked results_valid).  The first call after
// a scan that was ended by its summary reads the set's count words -- a word may still be on its way when the summary has
// arrived: the same bounded wait as psk_scan_end's, then fetch_counts and its tag check -- and they must add up to the
// summary's n_pass.  A set that is bound to a new scan before anyone asks is never read.
int held_seg_counts(psk_ctx *ctx, const std::vector<uint32_t> **counts)
{
    if (ctx->counts_pending) {
        const uint64_t n_summary = ctx->n_pass;
        const int set = ctx->res_set;
        PSK_TRY(wait_stamps(ctx, set, STAMP_WAIT_COUNTS));
        PSK_TRY(fetch_counts(ctx, set));
        if (ctx->n_pass != n_summary) {
            ctx->results_valid = false;
            return psk_fail(ctx, PSK_ESTATE, "the segments of scan %u hold %llu survivors, its summary said %llu", (uint32_t)ctx->slot[set].seq,
                            (unsigned long long)ctx->n_pass, (unsigned long long)n_summary);
        }
    }
    if (counts) *counts = &ctx->seg_counts;
    return PSK_OK;
}

// most workgroups of a scan launch: PSK_GRID_MULT (read by psk_init) per CU
uint64_t scan_grid_cap(const psk_ctx *ctx) { return (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : PSK_SC_GRID_MULT); }

dim3 scan_grid(const psk_ctx *ctx, uint64_t M, int G, int unroll, bool lut)
{
    // the table-in-LDS form: one 1024-thread workgroup per CU (its 64-120 KB of LDS admit no second one), and one
    // per result segment at least
    if (lut) return dim3((unsigned)std::max(SC_NSEG, ctx->n_cu > 0 ? ctx->n_cu : 256));
    const uint64_t rpw = sc_rpw(G);
    const uint64_t steps = (M + rpw - 1) / rpw;
    const uint64_t waves = (steps + unroll - 1) / unroll;
    uint64_t blocks = (waves + SC_THREADS / 64 - 1) / (SC_THREADS / 64);
    const uint64_t cap = scan_grid_cap(ctx);
    if (blocks > cap) blocks = cap;
    if (blocks < SC_NSEG) blocks = SC_NSEG;  // every result segment needs a workgroup to publish its count
    return dim3((unsigned)blocks);
}

// The result set the next scan writes: the one no scan in flight is writing; with none in flight, the one no
// asynchronous export (psk_export_survivors_async) is still reading and -- keep_results, the two-call form -- not the
// one that holds the last ended scan's results, so that the caller can launch the next scan BEFORE it reads those.
// If the set has an export pending, the scan waits for that export on the device.
int pick_result_set(psk_ctx *ctx, int *set_out, bool keep_results)
{
    int set;
    if (ctx->n_in_flight) set = ctx->slot[0].in_flight ? 1 : 0;
    else if (ctx->slot[ctx->res_set].export_pending || (keep_results && ctx->results_valid)) set = ctx->res_set ^ 1;
    else set = ctx->res_set;
    ScanSlot &sl = ctx->slot[set];
    if (sl.export_pending) {
        PSK_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.ev_export, 0));
        sl.export_pending = false;
    }
    if (!sl.ev0) {
        PSK_HIP(ctx, hipEventCreate(&sl.ev0));
        PSK_HIP(ctx, hipEventCreate(&sl.ev1));
    }
    *set_out = set;
    return PSK_OK;
}

namespace {

// one block per segment: copies the segment's entries to their place in the contiguous arrays
__global__ void pack_segments_kernel(const uint8_t *__restrict__ src, uint64_t cap, uint32_t seg_cap,
                                     const uint32_t *__restrict__ counts, const uint64_t *__restrict__ offsets,
                                     uint8_t *__restrict__ dst, uint64_t n, const uint64_t *__restrict__ union_words,
                                     uint64_t *__restrict__ words_out)
{
    const uint32_t seg = blockIdx.x;
    const uint32_t c = counts[seg];
    const uint64_t in0 = (uint64_t)seg * seg_cap, out0 = offsets[seg];
    const uint64_t *r = reinterpret_cast<const uint64_t *>(src);
    uint64_t *d = reinterpret_cast<uint64_t *>(dst);
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
#pragma unroll
        for (int f = 0; f < 5; f++) d[(uint64_t)f * n + out0 + i] = r[(uint64_t)f * cap + in0 + i];
        reinterpret_cast<int32_t *>(dst + 40 * n)[out0 + i] = reinterpret_cast<const int32_t *>(src + 40 * cap)[in0 + i];
        words_out[out0 + i] = union_words[r[in0 + i]];  // the k-mer word of the surviving row
    }
}

}  // namespace

extern "C" int psk_get_results(psk_ctx *ctx, uint64_t *row_idx, uint64_t *words, double *stat, double *p,
                               double *mean_x, double *mean_y, int32_t *n_with, uint64_t cap)
{
    if (!ctx) return PSK_EINVAL;
    if (!ctx->last_scan_kind) return psk_fail(ctx, PSK_ESTATE, "no scan has been run");
    if (!ctx->results_valid) return psk_fail(ctx, PSK_ESTATE, "no ended scan whose results are still held (psk_scan_end first)");
    const uint64_t n = ctx->n_pass;
    if (cap < n) return psk_fail(ctx, PSK_ERANGE, "buffer too small: %llu < %llu", (unsigned long long)cap,
                                 (unsigned long long)n);
    if (n == 0) return PSK_OK;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const std::vector<uint32_t> *seg_counts = nullptr;
    PSK_TRY(held_seg_counts(ctx, &seg_counts));
    // pack the segments into contiguous SoA arrays of n entries
    {
        std::vector<uint64_t> offs(SC_NSEG);
        uint64_t acc = 0;
        for (int sgm = 0; sgm < SC_NSEG; sgm++) { offs[sgm] = acc; acc += (*seg_counts)[sgm]; }
        PSK_TRY(dev_reserve(ctx, ctx->res_sorted, n * 52 + 128 + SC_NSEG * 12));
        uint8_t *aux = ctx->res_sorted.as<uint8_t>() + ((n * 52 + 63) & ~63ull);
        uint32_t *d_cnt = reinterpret_cast<uint32_t *>(aux + SC_NSEG * 8);
        PSK_HIP(ctx, hipMemcpyAsync(aux, offs.data(), SC_NSEG * 8, hipMemcpyHostToDevice, ctx->stream));
        PSK_HIP(ctx, hipMemcpyAsync(d_cnt, seg_counts->data(), SC_NSEG * 4, hipMemcpyHostToDevice, ctx->stream));
        pack_segments_kernel<<<SC_NSEG, 256, 0, ctx->stream>>>(ctx->slot[ctx->res_set].res.as<uint8_t>(), ctx->res_seg_cap * SC_NSEG,
                                                             (uint32_t)ctx->res_seg_cap, d_cnt,
                                                             reinterpret_cast<const uint64_t *>(aux),
                                                             ctx->res_sorted.as<uint8_t>(), n,
                                                             ctx->union_words.as<uint64_t>(),
                                                             reinterpret_cast<uint64_t *>(ctx->res_sorted.as<uint8_t>() + ((n * 44 + 7) & ~7ull)));
        PSK_HIP(ctx, hipGetLastError());
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const uint64_t c = n;
    const uint8_t *b = ctx->res_sorted.as<uint8_t>();
    std::vector<uint64_t> rows(n);
    std::vector<double> st(n), pv(n), mx(n), my(n);
    std::vector<int32_t> nw(n);
    PSK_HIP(ctx, hipMemcpy(rows.data(), b, n * 8, hipMemcpyDeviceToHost));
    PSK_HIP(ctx, hipMemcpy(st.data(), b + c * 8, n * 8, hipMemcpyDeviceToHost));
    PSK_HIP(ctx, hipMemcpy(pv.data(), b + c * 16, n * 8, hipMemcpyDeviceToHost));
    if (ctx->last_scan_kind == 2) {
        PSK_HIP(ctx, hipMemcpy(mx.data(), b + c * 24, n * 8, hipMemcpyDeviceToHost));
        PSK_HIP(ctx, hipMemcpy(my.data(), b + c * 32, n * 8, hipMemcpyDeviceToHost));
    }
    PSK_HIP(ctx, hipMemcpy(nw.data(), b + c * 40, n * 4, hipMemcpyDeviceToHost));
    // the append order of the scan is not deterministic: order by row (= ascending k-mer)
    std::vector<uint64_t> ord(n);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) { return rows[x] < rows[y]; });
    std::vector<uint64_t> wbuf;
    if (words) {  // gathered on the device by pack_segments_kernel, same (segment) order as the other columns
        wbuf.resize(n);
        PSK_HIP(ctx, hipMemcpy(wbuf.data(), b + ((n * 44 + 7) & ~7ull), n * 8, hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t j = ord[i];
        if (row_idx) row_idx[i] = rows[j];
        if (words) words[i] = wbuf[j];
        if (stat) stat[i] = st[j];
        if (p) p[i] = pv[j];
        if (mean_x) mean_x[i] = (ctx->last_scan_kind == 2) ? mx[j] : 0.0;
        if (mean_y) mean_y[i] = (ctx->last_scan_kind == 2) ? my[j] : 0.0;
        if (n_with) n_with[i] = nw[j];
    }
    return PSK_OK;
}

// one block per result segment: writes the segment's survivors as AoS records into a caller buffer.
// Segment offsets are computed on the device from the scan's own counters (no host round trip).
__global__ void export_records_kernel(const uint8_t *__restrict__ res, uint64_t cap, uint32_t seg_cap,
                                      const uint32_t *__restrict__ counters, const uint64_t *__restrict__ union_words,
                                      const uint64_t *__restrict__ bits, int wpr, uint64_t *__restrict__ dst,
                                      uint64_t cap_records)
{
    __shared__ uint32_t cnt[SC_NSEG];
    __shared__ uint64_t s_off, s_total;
    const uint32_t seg = blockIdx.x;
    cnt[threadIdx.x] = counters[threadIdx.x];  // the compact final counts; blockDim.x == SC_NSEG
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t off = 0, tot = 0;
        for (int j = 0; j < SC_NSEG; j++) { if (j == (int)seg) off = tot; tot += cnt[j]; }
        s_off = off;
        s_total = tot;
    }
    __syncthreads();
    const uint32_t c = cnt[seg];
    const uint64_t in0 = (uint64_t)seg * seg_cap, out0 = s_off;
    const uint64_t rec_words = 6 + (uint64_t)wpr;
    const uint64_t *f64s = reinterpret_cast<const uint64_t *>(res);  // row / stat / p / mx / my as raw 64-bit patterns
    const int32_t *nw = reinterpret_cast<const int32_t *>(res + 40 * cap);
    if (seg == 0 && threadIdx.x == 0) {  // header record: number of records that follow
        dst[0] = s_total;
        for (uint64_t j = 1; j < rec_words; j++) dst[j] = 0;
    }
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
        const uint64_t o = out0 + i;
        if (o >= cap_records) continue;
        uint64_t *rec = dst + (o + 1) * rec_words;
        const uint64_t r = f64s[in0 + i];
        rec[0] = union_words[r];
        rec[1] = f64s[1 * cap + in0 + i];
        rec[2] = f64s[2 * cap + in0 + i];
        rec[3] = f64s[3 * cap + in0 + i];
        rec[4] = f64s[4 * cap + in0 + i];
        rec[5] = (uint64_t)(int64_t)nw[in0 + i];
        for (int w = 0; w < wpr; w++) rec[6 + w] = bits[r * (uint64_t)wpr + w];
    }
}

extern "C" int psk_export_survivors(psk_ctx *ctx, void *device_dst, uint64_t cap_records, uint64_t *n_records)
{
    if (!ctx) return PSK_EINVAL;
    if (!ctx->last_scan_kind) return psk_fail(ctx, PSK_ESTATE, "no scan has been run");
    if (!ctx->results_valid) return psk_fail(ctx, PSK_ESTATE, "no ended scan whose results are still held (psk_scan_end first)");
    if (!device_dst || cap_records < 1) return psk_fail(ctx, PSK_EINVAL, "bad destination");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    PSK_TRY(held_seg_counts(ctx, nullptr));   // (the kernel reads the device's compact counts; the host's copy is checked as psk_scan_end used to)
    if (n_records) *n_records = ctx->n_pass;
    export_records_kernel<<<SC_NSEG, SC_NSEG, 0, ctx->stream>>>(
        ctx->slot[ctx->res_set].res.as<uint8_t>(), ctx->res_seg_cap * SC_NSEG, (uint32_t)ctx->res_seg_cap,
        ctx->res_count.as<uint32_t>() + SC_NSEG * SC_CNT_STRIDE + ctx->res_set * SC_NSEG, ctx->union_words.as<uint64_t>(), ctx->bits.as<uint64_t>(),
        ctx->wpr, static_cast<uint64_t *>(device_dst),
        cap_records);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

// The same export, queued on the CALLER's stream and not waited for: a collective queued on that stream next (RCCL
// all_gather_into_tensor) is ordered after it without a host synchronisation, and the next scan of this context
// waits (on the device) for the export before it overwrites the result arrays.
extern "C" int psk_export_survivors_async(psk_ctx *ctx, void *device_dst, uint64_t cap_records, void *stream)
{
    if (!ctx) return PSK_EINVAL;
    if (!ctx->last_scan_kind) return psk_fail(ctx, PSK_ESTATE, "no scan has been run");
    if (!ctx->results_valid) return psk_fail(ctx, PSK_ESTATE, "no ended scan whose results are still held (psk_scan_end first)");
    if (!device_dst || cap_records < 1) return psk_fail(ctx, PSK_EINVAL, "bad destination");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    PSK_TRY(held_seg_counts(ctx, nullptr));   // (the kernel reads the device's compact counts; the host's copy is checked as psk_scan_end used to)
    hipStream_t st = static_cast<hipStream_t>(stream);
    ScanSlot &sl = ctx->slot[ctx->res_set];
    // A scan that psk_scan_end waited for by its event has completed: its rows and counts are visible to any stream.  A
    // stamped scan has only published its words: the dispatch may not have retired, and its rows lie in the L2 of whichever
    // XCD appended them until it does.  The export runs on another stream, so it is ordered behind the scan on the device.
    // (The event also covers a later scan already queued on ctx->stream: hence exports_async, after which the scans of
    // this context carry their events again and this branch is not taken.)
    if (sl.stamped) {
        if (!sl.ev_ended) PSK_HIP(ctx, hipEventCreateWithFlags(&sl.ev_ended, hipEventDisableTiming));
        PSK_HIP(ctx, hipEventRecord(sl.ev_ended, ctx->stream));
        PSK_HIP(ctx, hipStreamWaitEvent(st, sl.ev_ended, 0));
    }
    ctx->exports_async = true;
    hipEvent_t &ev = sl.ev_export;
    if (!ev) PSK_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    export_records_kernel<<<SC_NSEG, SC_NSEG, 0, st>>>(
        ctx->slot[ctx->res_set].res.as<uint8_t>(), ctx->res_seg_cap * SC_NSEG, (uint32_t)ctx->res_seg_cap,
        ctx->res_count.as<uint32_t>() + SC_NSEG * SC_CNT_STRIDE + ctx->res_set * SC_NSEG, ctx->union_words.as<uint64_t>(), ctx->bits.as<uint64_t>(),
        ctx->wpr, static_cast<uint64_t *>(device_dst), cap_records);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipEventRecord(ev, st));
    ctx->slot[ctx->res_set].export_pending = true;
    return PSK_OK;
}

extern "C" double psk_last_scan_ms(const psk_ctx *ctx) { return ctx ? ctx->last_scan_ms : 0.0; }
