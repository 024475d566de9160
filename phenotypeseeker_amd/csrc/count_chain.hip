// a1: per-sample canonical k-mer list (replaces bin/glistmaker; modeling.py:303-315) -- the GPU half of one sample, as the
// batch driver (count_batch.hip) queues it on a buffer set ("lane"): chain_upload, chain_compute, chain_finalize.
//
//   device extract_kernel        2-bit encode, rolling forward/reverse words, canonical min,
//                                slab filter, per-wave LDS compaction + one reservation per wave
//          dev_radix_sort_u64    LSD radix sort on the 2k significant bits
//          rle_* kernels         run heads -> unique words + u32 frequencies
#include "dev_utils.h"
#include "kmer_windows.h"
#include "psk_internal.h"

// ------------------------------------------------------------------------------------------------
// Device kernels
// ------------------------------------------------------------------------------------------------
namespace {

// clean: bases and '\n' breaks, 16-byte aligned, padded with '\n' to a multiple of EX_SEG.
// Every lane rolls EX_SEG consecutive window ends; the wave compacts its valid words into its own
// 16 KiB LDS region (ballot ranks, wave-uniform running count); the workgroup reserves its output range
// with ONE atomic and every wave spills its region with consecutive lanes on consecutive addresses.
__global__ __launch_bounds__(EX_THREADS) void extract_kernel(const uint8_t *__restrict__ clean, uint64_t len, int k,
                                                              uint64_t lo, uint64_t hi, uint64_t *__restrict__ out,
                                                              uint32_t *__restrict__ n_out)
{
    __shared__ uint64_t stage[EX_THREADS / 64][64 * EX_SEG];
    const uint64_t g = (uint64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    const uint64_t s = g * EX_SEG;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t mask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const int rcshift = 2 * (k - 1);
    const bool active = s < len;

    uint32_t cur[EX_SEG / 4], prev[EX_HALO / 4];
#pragma unroll
    for (int j = 0; j < EX_SEG / 4; j++) cur[j] = 0x0a0a0a0au;
#pragma unroll
    for (int j = 0; j < EX_HALO / 4; j++) prev[j] = 0x0a0a0a0au;
    if (active) {
        const uint4 *p = reinterpret_cast<const uint4 *>(clean + s);
#pragma unroll
        for (int q = 0; q < EX_SEG / 16; q++) {
            const uint4 a = p[q];
            cur[4 * q] = a.x; cur[4 * q + 1] = a.y; cur[4 * q + 2] = a.z; cur[4 * q + 3] = a.w;
        }
        // the EX_HALO bytes before s, 16 at a time (what lies before the buffer counts as a break)
#pragma unroll
        for (int q = 0; q < EX_HALO / 16; q++) {
            const uint64_t back = (uint64_t)(EX_HALO / 16 - q) * 16;
            if (s >= back) {
                const uint4 c = *reinterpret_cast<const uint4 *>(clean + s - back);
                prev[4 * q] = c.x; prev[4 * q + 1] = c.y; prev[4 * q + 2] = c.z; prev[4 * q + 3] = c.w;
            }
        }
    }
    Roll r{0, 0, 0};
    // warm-up over the k-1 bytes before s (k-1 <= 31 < EX_HALO)
#pragma unroll
    for (int j = 0; j < EX_HALO; j++) {
        if (j >= EX_HALO - (k - 1)) {
            const uint32_t c = (prev[j >> 2] >> ((j & 3) * 8)) & 0xffu;
            roll_byte(r, c, mask, rcshift, k);
        }
    }
    uint32_t wcount = 0;  // wave-uniform
#pragma unroll
    for (int j = 0; j < EX_SEG; j++) {
        const uint32_t c = (cur[j >> 2] >> ((j & 3) * 8)) & 0xffu;
        roll_byte(r, c, mask, rcshift, k);
        const uint64_t w = (r.fw < r.rc) ? r.fw : r.rc;
        const bool valid = active && (s + j < len) && (r.run >= k) && (w >= lo) && (hi == 0 || w < hi);
        const uint64_t bal = __ballot(valid);
        if (valid) stage[wid][wcount + __popcll(bal & psk_lanemask_lt(lane))] = w;
        wcount += (uint32_t)__popcll(bal);
    }
    // ONE reservation per workgroup: same-address atomics retire at ~11 ns each, so one per wave (2441 for a
    // 5-Mbp sample) was 27 of the kernel's 45 us
    __shared__ uint32_t s_wcount[EX_THREADS / 64];
    __shared__ uint32_t s_base;
    if (lane == 0) s_wcount[wid] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < EX_THREADS / 64; w++) tot += s_wcount[w];
        s_base = tot ? atomicAdd(n_out, tot) : 0u;
    }
    __syncthreads();
    uint32_t base = s_base;
    for (int w = 0; w < wid; w++) base += s_wcount[w];
    for (uint32_t i = lane; i < wcount; i += 64) out[(uint64_t)base + i] = stage[wid][i];
}

// ---- run-length encoding of the sorted words: unique words + u32 counts ---------------------------
// Two passes over the sorted keys and one tiny scan instead of flags / scan / scatter / counts:
//   rle_tile_kernel   per tile of 4096 keys: number of run heads, position of the first head
//   rle_tile_scan     one workgroup: exclusive scan of the head counts (-> output offset of every tile, total =
//                     number of unique words) and a suffix minimum of the first-head positions (-> where the
//                     run that is open at the end of a tile ends)
//   rle_emit_kernel   per tile again: head h writes its word and (position of the next head - its position)
// A wave covers 16 rows of 64 consecutive keys; the heads of a row are one ballot, so ranks and "next head"
// positions are scalar bit operations on wave-uniform masks.
constexpr int RLE_THREADS = 256;
constexpr int RLE_ROWS = 16;
constexpr int RLE_WAVE_KEYS = 64 * RLE_ROWS;                    // 1024
constexpr int RLE_TILE = RLE_WAVE_KEYS * (RLE_THREADS / 64);    // 4096

__device__ __forceinline__ uint64_t rle_row_heads(const uint64_t *__restrict__ keys, uint64_t n, uint64_t i, uint64_t *key_out)
{
    bool head = false;
    uint64_t k = 0;
    if (i < n) {
        k = keys[i];
        head = (i == 0) || keys[i - 1] != k;
    }
    *key_out = k;
    return __ballot(head);
}

// n_dev != nullptr: the key count sits in device memory (<= n_host, which sizes the grid)
__global__ __launch_bounds__(RLE_THREADS) void rle_tile_kernel(const uint64_t *__restrict__ keys, uint64_t n_host,
                                                               const uint32_t *__restrict__ n_dev,
                                                               uint32_t *__restrict__ tile_cnt,
                                                               uint32_t *__restrict__ tile_first)
{
    const uint64_t n = n_dev ? (uint64_t)*n_dev : n_host;
    __shared__ uint32_t s_cnt[RLE_THREADS / 64], s_first[RLE_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * RLE_TILE + (uint64_t)wid * RLE_WAVE_KEYS;
    uint32_t cnt = 0, first = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < RLE_ROWS; r++) {
        uint64_t k;
        const uint64_t m = rle_row_heads(keys, n, base + (uint64_t)r * 64 + lane, &k);
        if (m && first == 0xffffffffu) first = (uint32_t)(base + (uint64_t)r * 64 + __builtin_ctzll(m));
        cnt += __popcll(m);
    }
    if (lane == 0) { s_cnt[wid] = cnt; s_first[wid] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, f = 0xffffffffu;
        for (int w = 0; w < RLE_THREADS / 64; w++) { c += s_cnt[w]; if (s_first[w] < f) f = s_first[w]; }
        tile_cnt[blockIdx.x] = c;
        tile_first[blockIdx.x] = f;
    }
}

// tile_cnt -> exclusive offsets (in place), tile_first -> position of the first head AFTER the tile (in place),
// total[0] = number of heads
__global__ __launch_bounds__(1024) void rle_tile_scan_kernel(uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ tile_first,
                                                              uint32_t n_tiles, uint32_t n_host, const uint32_t *__restrict__ n_dev,
                                                              uint32_t *__restrict__ total)
{
    const uint32_t n = n_dev ? *n_dev : n_host;
    __shared__ uint32_t lds[16];
    __shared__ uint32_t s_min[16];
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 1024) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t v = t < n_tiles ? tile_cnt[t] : 0u;
        uint32_t all;
        const uint32_t ex = psk_block_excl_scan_u32<1024>(v, &all, lds);
        if (t < n_tiles) tile_cnt[t] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) total[0] = carry;
    // suffix minimum, exclusive: next[t] = min(first[t+1 ..]) or n; chunks from the back
    uint32_t tail = n;  // minimum over everything behind the current chunk
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t done = 0; done < n_tiles; done += 1024) {
        const uint32_t hi = n_tiles - done;                 // chunk = [lo, hi)
        const uint32_t lo = hi > 1024 ? hi - 1024 : 0;
        const uint32_t t = lo + threadIdx.x;
        const uint32_t v = t < hi ? tile_first[t] : 0xffffffffu;
        // inclusive suffix min within the wave (towards higher lanes), then across waves
        uint32_t m = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_down(m, d, 64);
            if (lane + d < 64 && o < m) m = o;
        }
        __syncthreads();
        if (lane == 0) s_min[wid] = m;  // minimum of the whole wave
        __syncthreads();
        uint32_t behind = tail;          // minimum of the waves behind this one + earlier chunks
        for (int w = wid + 1; w < 16; w++) if (s_min[w] < behind) behind = s_min[w];
        // exclusive: the inclusive suffix min of the next lane (or `behind` for the last lane)
        uint32_t nxt = __shfl_down(m, 1, 64);
        if (lane == 63) nxt = 0xffffffffu;
        uint32_t res = nxt < behind ? nxt : behind;
        uint32_t chunk_min = tail;
        for (int w = 0; w < 16; w++) if (s_min[w] < chunk_min) chunk_min = s_min[w];
        if (t < hi) tile_first[t] = res;
        tail = chunk_min;
        __syncthreads();
    }
}

__global__ __launch_bounds__(RLE_THREADS) void rle_emit_kernel(const uint64_t *__restrict__ keys, uint64_t n,
                                                               const uint32_t *__restrict__ tile_off,
                                                               const uint32_t *__restrict__ tile_next,
                                                               uint64_t *__restrict__ words, uint32_t *__restrict__ freqs)
{
    __shared__ uint32_t s_cnt[RLE_THREADS / 64], s_first[RLE_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * RLE_TILE + (uint64_t)wid * RLE_WAVE_KEYS;
    uint64_t mask[RLE_ROWS], key[RLE_ROWS];
    uint32_t cnt = 0, first = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < RLE_ROWS; r++) {
        mask[r] = rle_row_heads(keys, n, base + (uint64_t)r * 64 + lane, &key[r]);
        if (mask[r] && first == 0xffffffffu) first = (uint32_t)(base + (uint64_t)r * 64 + __builtin_ctzll(mask[r]));
        cnt += __popcll(mask[r]);
    }
    if (lane == 0) { s_cnt[wid] = cnt; s_first[wid] = first; }
    __syncthreads();
    uint32_t out = tile_off[blockIdx.x];
    for (int w = 0; w < wid; w++) out += s_cnt[w];
    // first head behind this wave: a later wave of the tile, else the first head after the tile
    uint32_t after = tile_next[blockIdx.x];
    for (int w = RLE_THREADS / 64 - 1; w > wid; w--) if (s_first[w] != 0xffffffffu) after = s_first[w];
    // position of the first head in a later row of this wave, per row (scalar, back to front)
    uint32_t later[RLE_ROWS];
    uint32_t nxt = after;
#pragma unroll
    for (int r = RLE_ROWS - 1; r >= 0; r--) {
        later[r] = nxt;
        if (mask[r]) nxt = (uint32_t)(base + (uint64_t)r * 64 + __builtin_ctzll(mask[r]));
    }
#pragma unroll
    for (int r = 0; r < RLE_ROWS; r++) {
        const uint64_t m = mask[r];
        if ((m >> lane) & 1) {
            const uint32_t pos = (uint32_t)(base + (uint64_t)r * 64 + lane);
            const uint64_t above = (lane == 63) ? 0ull : (m >> (lane + 1));
            const uint32_t next = above ? pos + 1 + (uint32_t)__builtin_ctzll(above) : later[r];
            const uint32_t j = out + __popcll(m & psk_lanemask_lt(lane));
            words[j] = key[r];
            freqs[j] = next - pos;
        }
        out += __popcll(m);
    }
}

}  // namespace

int launch_extract(psk_ctx *ctx, const uint8_t *clean, uint64_t len, int k, uint64_t lo, uint64_t hi, uint64_t *out,
                   uint32_t *n_out)
{
    if (len == 0) return PSK_OK;
    const uint64_t threads = (len + EX_SEG - 1) / EX_SEG;
    extract_kernel<<<div_up(threads, EX_THREADS), EX_THREADS, 0, ctx->stream>>>(clean, len, k, lo, hi, out, n_out);
    PSK_HIP(ctx, hipGetLastError());
    return PSK_OK;
}

// ---- the buffer sets and the three chain stages (the loop that drives them: BatchRun, count_batch.hip) -----------------------
static int lane_prepare(psk_ctx *ctx, CountLane &L)
{
    if (!L.done) {
        PSK_HIP(ctx, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        PSK_HIP(ctx, hipEventCreateWithFlags(&L.raw_ready, hipEventDisableTiming));
        PSK_HIP(ctx, hipEventCreateWithFlags(&L.raw_free, hipEventDisableTiming));
        PSK_HIP(ctx, hipEventCreateWithFlags(&L.up_done, hipEventDisableTiming));
    }
    if (!L.pinned_cnt) PSK_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&L.pinned_cnt), 64, hipHostMallocDefault));
    if (!ctx->copy_stream || !ctx->frame_stream) {
        // A process's first upload: the streams of the ingest.  hipStreamCreate costs ~7.5 ms apiece (a hardware queue), and all
        // five of r03 (copy + three more + framing, whatever PSK_COPY_STREAMS said) were created here one after the other: 40 of
        // the 55 ms of a process's first counting call (r04, PSK_TRACE).  Only the copy streams in use now, and together
        std::vector<hipStream_t *> want;
        if (!ctx->copy_stream) want.push_back(&ctx->copy_stream);
        for (int c = 0; c + 1 < ctx->copy_streams && c < 3; c++) if (!ctx->copy_more[c]) want.push_back(&ctx->copy_more[c]);
        if (!ctx->frame_stream) want.push_back(&ctx->frame_stream);
        std::vector<hipError_t> err(want.size(), hipSuccess);
        std::vector<std::thread> th;
        for (size_t q = 1; q < want.size(); q++)
            th.emplace_back([&, q] {
                err[q] = hipSetDevice(ctx->device);
                if (err[q] == hipSuccess) err[q] = hipStreamCreateWithFlags(want[q], hipStreamNonBlocking);
            });
        if (!want.empty()) err[0] = hipStreamCreateWithFlags(want[0], hipStreamNonBlocking);
        for (auto &t : th) t.join();
        for (hipError_t e : err)
            if (e != hipSuccess) return psk_fail(ctx, PSK_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    return PSK_OK;
}

// A grouped batch rotates 3 G buffer sets of eight device buffers each: carved out of ONE allocation (and one pinned block
// for the sets' counters) sized for the batch's longest sample, instead of ~170 hipMallocs on a cold context.  Buffers a
// set already owns and that are large enough stay as they are.  Nothing of an earlier batch is in flight here.
enum { LB_DC_CNT = 5, LANE_BUFS = 8 };   // (the counter ring among them: a fresh one is zeroed before its first use)
static void lane_bufs(CountLane &L, DevBuf *out[LANE_BUFS])
{
    DevBuf *b[LANE_BUFS] = {&L.raw, &L.rawin, &L.fr_scratch, &L.dc_part, &L.dc_wgoff, &L.dc_cnt, &L.dc_meta, &L.dc_mtemp};
    for (int q = 0; q < LANE_BUFS; q++) out[q] = b[q];
}
// what a buffer of `w` wanted bytes takes of the slab
static inline size_t slice_bytes(size_t w) { return (w + w / 8 + 511) & ~size_t(255); }

// what each buffer of a set wants for a longest sample of max_len bytes; returns the bytes of the set's slice of the slab
static size_t lane_set_wants(psk_ctx *ctx, size_t max_len, bool gpu_framing, size_t want[LANE_BUFS])
{
    size_t dcb[5];
    if (ctx->dense_mode) dense_lane_bytes(ctx, max_len, dcb);
    else bucket_lane_bytes(ctx, max_len, dcb);
    const size_t w[LANE_BUFS] = {max_len + 128 + 2 * EX_SEG, gpu_framing ? max_len + 64 : 0, gpu_framing ? frame_gpu_scratch_bytes(max_len) : 0,
                                 dcb[0], dcb[1], dcb[2], dcb[3], dcb[4]};
    size_t per_lane = 0;
    for (int q = 0; q < LANE_BUFS; q++) { want[q] = w[q]; per_lane += slice_bytes(w[q]); }
    return per_lane;
}
// bytes of ONE buffer set of a grouped batch whose longest sample has max_len bytes
size_t lane_set_bytes(psk_ctx *ctx, size_t max_len, bool gpu_framing)
{
    size_t want[LANE_BUFS];
    return lane_set_wants(ctx, max_len, gpu_framing, want);
}
// the slices carved out of the slab are forgotten (before a new layout, and when psk_begin gives a large slab back)
void psk_forget_lane_slices(psk_ctx *ctx)
{
    for (CountLane &L : ctx->lane) {
        DevBuf *b[LANE_BUFS];
        lane_bufs(L, b);
        for (int q = 0; q < LANE_BUFS; q++)
            if (b[q]->borrowed) { b[q]->p = nullptr; b[q]->cap = 0; b[q]->borrowed = false; }
    }
}

int carve_lanes(psk_ctx *ctx, int n_lanes, size_t max_len, bool gpu_framing)
{
    size_t want[LANE_BUFS];
    const size_t per_lane = lane_set_wants(ctx, max_len, gpu_framing, want);
    const size_t total = per_lane * (size_t)n_lanes;
    auto lacks = [&](const DevBuf *b, int q) { return want[q] && !(b->p && b->cap >= want[q]); };
    bool need = false;
    for (int l = 0; l < n_lanes && !need; l++) {
        DevBuf *b[LANE_BUFS];
        lane_bufs(ctx->lane[l], b);
        for (int q = 0; q < LANE_BUFS; q++) need = need || lacks(b[q], q);
    }
    if (need) {
        // a new layout: every buffer carved out of the slab so far is forgotten first (the slices of two layouts overlap)
        psk_forget_lane_slices(ctx);
        PSK_TRY(dev_reserve(ctx, ctx->lane_slab, total));
        // carve: set l takes slice l; a buffer that is its set's own and large enough is left alone
        for (int l = 0; l < n_lanes; l++) {
            DevBuf *b[LANE_BUFS];
            lane_bufs(ctx->lane[l], b);
            size_t off = per_lane * (size_t)l;
            for (int q = 0; q < LANE_BUFS; q++) {
                const size_t sz = slice_bytes(want[q]);
                if (lacks(b[q], q)) {
                    if (b[q]->p && !b[q]->borrowed) (void)hipFree(b[q]->p);
                    b[q]->p = static_cast<uint8_t *>(ctx->lane_slab.p) + off;
                    b[q]->cap = sz;
                    b[q]->borrowed = true;
                    if (q == LB_DC_CNT) ctx->lane[l].dc_slot = 0;   // a fresh counter ring: zeroed before its first use
                }
                off += sz;
            }
        }
    }
    if (!ctx->lane_pinned) PSK_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->lane_pinned), (size_t)16 * 4 * psk_ctx::LANES, hipHostMallocDefault));
    for (int l = 0; l < n_lanes; l++)
        if (!ctx->lane[l].pinned_cnt) ctx->lane[l].pinned_cnt = ctx->lane_pinned + 16 * l;
    return PSK_OK;
}

// Stage A of a sample on buffer set L, on the copy stream: the upload and, for raw file bytes (format 1 FASTA,
// 2 FASTQ; frame_gpu.hip), the framing kernels that turn them into the clean stream.  format 0: `src` is a clean
// stream the host framed, `bytes` its padded length.  L.raw_ready fires when the clean stream is in L.raw.
int chain_upload(psk_ctx *ctx, CountLane &L, const uint8_t *src, uint64_t bytes, int format, bool src_on_device)
{
    PSK_TRY(lane_prepare(ctx, L));
    if (bytes == 0) return PSK_OK;
    if (bytes >= (1ull << 32)) return psk_fail(ctx, PSK_ERANGE, "sample larger than 4 GB");
    const int which = (int)((&L - ctx->lane) % ctx->copy_streams);
    hipStream_t cs = which ? ctx->copy_more[which - 1] : ctx->copy_stream;
    // after the last reader of this set's clean stream (the sample before last)
    if (L.raw_used) PSK_HIP(ctx, hipStreamWaitEvent(cs, L.raw_free, 0));
    if (format == 0) {
        PSK_TRY(dev_reserve(ctx, L.raw, bytes));
        PSK_HIP(ctx, hipMemcpyAsync(L.raw.p, src, bytes, hipMemcpyHostToDevice, cs));
    } else {
        PSK_TRY(dev_reserve(ctx, L.rawin, bytes + 64));
        PSK_TRY(dev_reserve(ctx, L.raw, bytes + 128));
        PSK_TRY(dev_reserve(ctx, L.fr_scratch, frame_gpu_scratch_bytes(bytes)));
        PSK_HIP(ctx, hipMemcpyAsync(L.rawin.p, src, bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cs));   // (a .gz sample: its text was inflated on the device)
        // the framing kernels run on their own stream: the copy stream goes on with the next sample's upload (PCIe is
        // the slowest stage of the ingest: ~100 us per 5-Mbp sample against ~25 us of framing and ~60 us of counting)
        PSK_HIP(ctx, hipEventRecord(L.up_done, cs));
        PSK_HIP(ctx, hipStreamWaitEvent(ctx->frame_stream, L.up_done, 0));
        PSK_TRY(frame_gpu_enqueue(ctx, ctx->frame_stream, format, L.rawin.as<uint8_t>(), bytes, L.raw.as<uint8_t>(), L.fr_scratch.p,
                                  lane_frame_result(L)));
        PSK_HIP(ctx, hipEventRecord(L.raw_ready, ctx->frame_stream));
        return PSK_OK;
    }
    PSK_HIP(ctx, hipEventRecord(L.raw_ready, cs));
    return PSK_OK;
}

// the buffers of the radix route (and of the bucketed sort's fall-back onto it)
static int radix_lane_reserve(psk_ctx *ctx, CountLane &L, uint64_t n)
{
    PSK_TRY(dev_reserve(ctx, L.keysA, n * 8));
    PSK_TRY(dev_reserve(ctx, L.keysB, n * 8));
    PSK_TRY(dev_reserve(ctx, L.starts, (size_t)div_up(n, RLE_TILE) * 8));  // tile offsets | next-head positions
    PSK_TRY(dev_reserve(ctx, L.cnt, (size_t)CountLane::CNT_SLOTS * 16));
    return PSK_OK;
}

// The RLE count pair on the sorted keys: run heads per tile, then the one-workgroup scan, which leaves the number of unique
// words in slot[1].  n_dev != nullptr: the key count sits in device memory (<= n, which sizes the grid).  The layout of the
// tile arrays follows L.n (the emit pass of chain_finalize reads them by it).
static int rle_count(psk_ctx *ctx, CountLane &L, const uint64_t *sorted, uint64_t n, const uint32_t *n_dev, uint32_t *slot)
{
    if (n == 0) return PSK_OK;
    const uint32_t n_tiles = (uint32_t)div_up(n, RLE_TILE);
    uint32_t *t_off = L.starts.as<uint32_t>(), *t_next = t_off + div_up(L.n, RLE_TILE);
    rle_tile_kernel<<<n_tiles, RLE_THREADS, 0, ctx->stream>>>(sorted, n, n_dev, t_off, t_next);
    PSK_HIP(ctx, hipGetLastError());
    rle_tile_scan_kernel<<<1, 1024, 0, ctx->stream>>>(t_off, t_next, n_tiles, (uint32_t)n, n_dev, slot + 1);
    PSK_HIP(ctx, hipGetLastError());
    return PSK_OK;
}

// this sample's list is complete
static inline void list_complete(SampleList &S, uint64_t n_unique, uint64_t n_kept)
{
    S.n_unique = n_unique;
    S.n_total = n_kept;
    S.done = true;
}

// Stage B: the counting chain of the sample whose clean stream stage A put (or is putting) into L.raw.
// n = number of k-base windows (exact from the host's framing; the clean length, an upper bound, after the GPU's).
int chain_compute(psk_ctx *ctx, CountLane &L, int sample_idx, uint64_t clean_len, uint64_t n, bool n_exact)
{
    ctx->lists[sample_idx] = SampleList();
    ctx->have_presence = false;
    if (clean_len >= (1ull << 32)) return psk_fail(ctx, PSK_ERANGE, "sample larger than 4 Gbases");
    L.sample = sample_idx;
    L.n = n;
    L.exact = n_exact && ctx->slab_lo == 0 && ctx->slab_hi == 0;  // no slab filter: every window yields a word
    L.uniq = nullptr;
    L.dense = false;
    L.bs = false;
    if (n == 0) {
        if (ctx->dense_mode) {   // an empty sample still owns a (zero) bitmap: the presence build reads every sample's
            SampleList &S = ctx->lists[sample_idx];
            const size_t bytes = (size_t)ctx->dense_nb * DC_BUCKET_WORDS * 8;
            PSK_TRY(arena_alloc(ctx, bytes, (void **)&S.bitmap));
            PSK_HIP(ctx, hipMemsetAsync(S.bitmap, 0, bytes, ctx->stream));
            S.dense = true;
        }
        return PSK_OK;
    }
    PSK_HIP(ctx, hipStreamWaitEvent(ctx->stream, L.raw_ready, 0));
    if (ctx->dense_mode) {   // 2k <= 26: no sort (dense_count.hip)
        if (ctx->dense_defer && dense_group_ok(ctx, n)) {   // a genome of a batch: its chain is launched with its group's
            L.group_pending = true;
            L.clean_len = clean_len;
            return PSK_OK;
        }
        return dense_chain_enqueue(ctx, L, sample_idx, clean_len, n);
    }
    if (bucket_route_ok(ctx, n)) {   // k = 14..16, splitters known
        if (ctx->dense_defer) {      // a genome of a batch: its chain is launched with its group's
            L.group_pending = true;
            L.clean_len = clean_len;
            return PSK_OK;
        }
        return bucket_chain_enqueue(ctx, L, sample_idx, clean_len, n);
    }
    PSK_TRY(radix_lane_reserve(ctx, L, n));
    // every sample takes a fresh pre-zeroed counter slot (a 16-byte memset per sample is a 6 us launch)
    if (L.cnt_slot == 0 || L.cnt_slot >= CountLane::CNT_SLOTS) {
        PSK_HIP(ctx, hipMemsetAsync(L.cnt.p, 0, (size_t)CountLane::CNT_SLOTS * 16, ctx->stream));
        L.cnt_slot = 0;
    }
    uint32_t *d_n = L.cnt.as<uint32_t>() + 4 * (size_t)L.cnt_slot++;
    PSK_TRY(launch_extract(ctx, L.raw.as<uint8_t>(), clean_len, ctx->k, ctx->slab_lo, ctx->slab_hi, L.keysA.as<uint64_t>(),
                           d_n));
    PSK_HIP(ctx, hipEventRecord(L.raw_free, ctx->stream));
    L.raw_used = true;
    uint64_t *sorted = nullptr;
    // with a slab filter only the GPU knows how many words were kept: the launches cover the host's count
    // (every window) and the kernels read the real one from d_n[0]
    const uint32_t *n_dev = L.exact ? nullptr : d_n;
    PSK_TRY(dev_radix_sort_u64(ctx, L.keysA.as<uint64_t>(), L.keysB.as<uint64_t>(), n, 0, 2 * ctx->k, &sorted, n_dev));
    PSK_TRY(rle_count(ctx, L, sorted, n, n_dev, d_n));
    PSK_HIP(ctx, hipMemcpyAsync(L.pinned_cnt, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    PSK_HIP(ctx, hipEventRecord(L.done, ctx->stream));
    L.uniq = sorted;  // the emit pass (chain_finalize) reads the sorted keys once the output size is known
    return PSK_OK;
}

// second half: arena allocation + the emit pass (straight into the arena) of the sample whose chain ran on this set
int chain_finalize(psk_ctx *ctx, CountLane &L)
{
    if (L.sample < 0) return PSK_OK;
    SampleList &S = ctx->lists[L.sample];
    const int sample = L.sample;
    const uint64_t windows = L.n;
    L.sample = -1;
    uint64_t nu = 0, n_kept = 0;
    if (L.n > 0) {
        PSK_HIP(ctx, hipEventSynchronize(L.done));
        const uint64_t n_gpu = L.pinned_cnt[0];
        if (L.exact ? (n_gpu != L.n) : (n_gpu > L.n))
            return psk_fail(ctx, PSK_ESTATE, "sample %d: the GPU kept %llu windows, the framing counted %llu", sample,
                            (unsigned long long)n_gpu, (unsigned long long)L.n);
        n_kept = n_gpu;
        nu = L.pinned_cnt[1];
        if (L.dense) {
            L.sample = sample;
            const int rc = dense_chain_finalize(ctx, L, &n_kept, &nu);
            L.sample = -1;
            if (rc != PSK_OK) return rc;
            list_complete(S, nu, n_kept);
            return PSK_OK;
        }
        if (L.bs) {
            bool fell_back = false;
            PSK_TRY(bucket_chain_finalize(ctx, L, S, n_kept, nu, &fell_back));
            if (!fell_back) {
                list_complete(S, nu, n_kept);
                return PSK_OK;
            }
            // a bucket outgrew the LDS sort: the partitioned words through the radix sort and the run-length passes, waited for
            // (rare: a sample unlike the one the splitters were taken from)
            uint64_t *sorted = nullptr;
            L.dc_defer_compact = false;   // (in a group: this sample's list is made here, not by the group's packing launch)
            PSK_TRY(radix_lane_reserve(ctx, L, L.n));
            PSK_TRY(bucket_fallback_keys(ctx, L, n_kept, L.keysA.as<uint64_t>()));
            PSK_TRY(dev_radix_sort_u64(ctx, L.keysA.as<uint64_t>(), L.keysB.as<uint64_t>(), n_kept, 0, 2 * ctx->k, &sorted, nullptr));
            uint32_t *d_n = L.cnt.as<uint32_t>() + 4 * (size_t)(CountLane::CNT_SLOTS - 1);
            PSK_TRY(rle_count(ctx, L, sorted, n_kept, nullptr, d_n));
            PSK_HIP(ctx, hipMemcpyAsync(L.pinned_cnt + 1, d_n + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
            PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            nu = n_kept ? L.pinned_cnt[1] : 0;
            L.uniq = sorted;
        }
        PSK_TRY(arena_alloc(ctx, nu * 8, (void **)&S.words));
        PSK_TRY(arena_alloc(ctx, nu * 4, (void **)&S.freqs));
        const uint32_t n_tiles = (uint32_t)div_up(L.n, RLE_TILE);  // the layout of the tile arrays follows L.n
        const uint32_t *t_off = L.starts.as<uint32_t>();
        if (n_kept)
            rle_emit_kernel<<<(uint32_t)div_up(n_kept, RLE_TILE), RLE_THREADS, 0, ctx->stream>>>(L.uniq, n_kept, t_off, t_off + n_tiles,
                                                                                        S.words, S.freqs);
        PSK_HIP(ctx, hipGetLastError());
    }
    list_complete(S, nu, n_kept);
    PSK_TRY(bucket_splitters_from(ctx, S, windows));   // k = 14..16: the later samples of the run take the bucketed sort
    return PSK_OK;
}

int ensure_pinned(psk_ctx *ctx, void **buf, size_t *cap, size_t need)
{
    if (need <= *cap && *buf) return PSK_OK;
    pinned_release(ctx, *buf, *cap);   // (r06: pinned buffers come from, and go back to, a process-wide cache: api.hip)
    *buf = nullptr;
    *cap = 0;
    return pinned_acquire(ctx, need, buf, cap);
}

// frame into the context's single pinned buffer and upload (dictionary counting, MinHash)
int upload_clean(psk_ctx *ctx, const uint8_t *bytes, size_t len, uint64_t *clean_len)
{
    PSK_TRY(ensure_pinned(ctx, &ctx->pinned, &ctx->pinned_cap, len + 2 * EX_SEG));
    uint64_t padded = 0;
    int rc = frame_into(static_cast<uint8_t *>(ctx->pinned), ctx->pinned_cap, bytes, len, clean_len, &padded);
    if (rc) return psk_fail(ctx, rc, "framing failed");
    PSK_TRY(dev_reserve(ctx, ctx->raw, padded));
    PSK_HIP(ctx, hipMemcpyAsync(ctx->raw.p, ctx->pinned, padded, hipMemcpyHostToDevice, ctx->stream));
    return PSK_OK;
}
