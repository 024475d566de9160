// Exception-coded copy of the presence matrix for the unweighted chi2 scan (assoc_scan.hip chi2_scan_kernel_cx).
//
// A k-mer union of bacterial genomes is core-or-rare: at config 2 (256 x 5 Mbp, k = 13) 91.5 % of the rows differ from
// all-absent or all-present in at most 7 samples.  Such a row needs one 8-byte slot -- a header byte (e = the number of
// exceptions, whether they are the present or the absent samples) and the exceptions' sample indices as u8 -- against a
// 32-byte dense row.  Rows with more exceptions are flagged in their slot and copied, ascending, into a side matrix of
// dense rows with their row ids.  The scan then streams 8 B per row plus the side matrix (about 0.35 of the dense bytes
// at config 2) and reads nothing else per row.  The dense matrix stays as it is: every other reader uses it.
//
// Two passes over the dense matrix: the first counts the overflow rows of every workgroup (whose exclusive scan places
// them), the host decides from the total whether to keep a copy (CX_MAX_SHARE, CX_MAX_OVF_DIV), the second writes slots and side matrix.
// Beside each side-matrix row the encoder keeps its popcount (cx_ov_pc, u16) and, on the host, how many rows have each
// popcount (cx_pc_hist): a scan's parameters rule out whole popcounts (cx_pc_plan, chi2_plan.h), and the scan then
// reads 2 bytes of such a row instead of the row.
// Which rows have a given popcount is the matrix's too, so the encoder also groups the rows' positions by popcount
// (cx_pc_index, u32; bucket pc starts at the exclusive prefix of the histogram, cx_pc_start on the host): a scan whose
// feasible popcounts hold few rows visits those alone (chi2_scan_kernel_cx_side_idx).
// PSK_TRACE=1 prints the decision, the time of the build, the popcounts' non-zero range and the time of the index.
#include "dev_utils.h"
#include "psk_internal.h"

#include <algorithm>
#include <chrono>

namespace {

constexpr int CX_THREADS = 256;
typedef unsigned long long cx_u64x2 __attribute__((ext_vector_type(2)));

// the row's words (wpr = 2 or 4), restricted to the n valid samples
__device__ __forceinline__ int cx_load_row(const uint64_t *__restrict__ bits, uint64_t r, int wpr, int n, uint64_t w[4])
{
    const cx_u64x2 *p = reinterpret_cast<const cx_u64x2 *>(bits + r * (uint64_t)wpr);
    const cx_u64x2 a = p[0];
    const cx_u64x2 b = wpr == 4 ? p[1] : (cx_u64x2){0ull, 0ull};
    w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
    int pc = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int valid = n - 64 * c;
        w[c] &= valid <= 0 ? 0ull : valid >= 64 ? ~0ull : (1ull << valid) - 1ull;
        pc += __popcll(w[c]);
    }
    return pc;
}

__global__ __launch_bounds__(CX_THREADS) void cx_count_kernel(const uint64_t *__restrict__ bits, uint64_t M, int wpr, int n,
                                                             uint32_t *__restrict__ counts)
{
    const uint64_t r = (uint64_t)blockIdx.x * CX_THREADS + threadIdx.x;
    bool ovf = false;
    if (r < M) {
        uint64_t w[4];
        const int pc = cx_load_row(bits, r, wpr, n, w);
        ovf = min(pc, n - pc) > CX_MAX_E;
    }
    const int cnt = __syncthreads_count(ovf);
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)cnt;
}

// offs: exclusive scan of cx_count_kernel's counts (same grid)
__global__ __launch_bounds__(CX_THREADS) void cx_encode_kernel(const uint64_t *__restrict__ bits, uint64_t M, int wpr, int n,
                                                              const uint32_t *__restrict__ offs, uint64_t *__restrict__ slots,
                                                              uint64_t *__restrict__ ov, uint32_t *__restrict__ ov_row,
                                                              uint16_t *__restrict__ ov_pc)
{
    __shared__ uint32_t s_wave[CX_THREADS / 64];
    const uint64_t r = (uint64_t)blockIdx.x * CX_THREADS + threadIdx.x;
    uint64_t w[4] = {0ull, 0ull, 0ull, 0ull};
    int pc = 0;
    if (r < M) pc = cx_load_row(bits, r, wpr, n, w);
    const bool absent = pc > n - pc;           // the exceptions are the absent samples
    const int e = absent ? n - pc : pc;
    const bool ovf = r < M && e > CX_MAX_E;
    uint32_t total;
    const uint32_t pos = psk_block_excl_scan_u32<CX_THREADS>(ovf ? 1u : 0u, &total, s_wave);   // ascending within the workgroup
    if (r >= M) return;
    if (ovf) {
        const uint64_t j = (uint64_t)offs[blockIdx.x] + pos;
        for (int c = 0; c < wpr; c++) ov[j * wpr + c] = w[c];
        ov_row[j] = (uint32_t)r;
        ov_pc[j] = (uint16_t)pc;
        slots[r] = CX_HDR_OVF;
        return;
    }
    uint64_t slot = (uint64_t)e | (absent ? CX_HDR_BASE : 0u);
    int k = 1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int valid = n - 64 * c;
        uint64_t x = absent ? ~w[c] & (valid <= 0 ? 0ull : valid >= 64 ? ~0ull : (1ull << valid) - 1ull) : w[c];
        while (x) {   // at most CX_MAX_E bits over the whole row
            slot |= (uint64_t)(64 * c + __builtin_ctzll(x)) << (8 * k);
            k++;
            x &= x - 1;
        }
    }
    slots[r] = slot;
}

// hist[pc] += rows of that popcount: a histogram per workgroup in LDS, then one global atomic per non-empty bin
constexpr int CX_HIST_BINS = CX_MAX_SAMPLES + 1;
__global__ __launch_bounds__(CX_THREADS) void cx_pc_hist_kernel(const uint16_t *__restrict__ ov_pc, uint64_t n_ov, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[CX_HIST_BINS];
    for (int i = threadIdx.x; i < CX_HIST_BINS; i += CX_THREADS) s_hist[i] = 0;
    __syncthreads();
    for (uint64_t j = (uint64_t)blockIdx.x * CX_THREADS + threadIdx.x; j < n_ov; j += (uint64_t)gridDim.x * CX_THREADS) {
        const uint32_t pc = ov_pc[j];
        atomicAdd(&s_hist[pc < CX_HIST_BINS ? pc : CX_HIST_BINS - 1], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CX_HIST_BINS; i += CX_THREADS)
        if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

// cursor[pc] = rows of a smaller popcount: the exclusive scan of the histogram, one workgroup (bin 256, the last, starts
// at the total of the others)
static_assert(CX_HIST_BINS == CX_THREADS + 1, "one bin per thread and the last from the total");
__global__ __launch_bounds__(CX_THREADS) void cx_pc_start_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ cursor)
{
    __shared__ uint32_t s_wave[CX_THREADS / 64];
    uint32_t total;
    const uint32_t pos = psk_block_excl_scan_u32<CX_THREADS>(hist[threadIdx.x], &total, s_wave);
    cursor[threadIdx.x] = pos;
    if (threadIdx.x == 0) cursor[CX_THREADS] = total;
}

// index = the rows' positions grouped by popcount, as cx_pc_hist_kernel counts them: a workgroup histograms its tile of
// CX_INDEX_TILE rows in LDS, reserves its share of every non-empty bucket with ONE global atomic per bin (the popcounts
// pile into a few bins: one atomic per row on a bucket's cursor would serialise), and places its rows with the cursors
// in LDS.  cursor: cx_pc_start_kernel's, so a bucket's last position is start + rows of that popcount - 1 < n_ov.
constexpr int CX_INDEX_PER_THREAD = 16, CX_INDEX_TILE = CX_THREADS * CX_INDEX_PER_THREAD;
__global__ __launch_bounds__(CX_THREADS) void cx_pc_index_kernel(const uint16_t *__restrict__ ov_pc, uint64_t n_ov, uint32_t *__restrict__ cursor,
                                                                uint32_t *__restrict__ index)
{
    __shared__ uint32_t s_cur[CX_HIST_BINS];
    for (int i = threadIdx.x; i < CX_HIST_BINS; i += CX_THREADS) s_cur[i] = 0;
    __syncthreads();
    const uint64_t j0 = (uint64_t)blockIdx.x * CX_INDEX_TILE + threadIdx.x;
    uint32_t pc[CX_INDEX_PER_THREAD];
#pragma unroll
    for (int u = 0; u < CX_INDEX_PER_THREAD; u++) {
        const uint64_t j = j0 + (uint64_t)u * CX_THREADS;
        pc[u] = 0;
        if (j < n_ov) {
            const uint32_t v = ov_pc[j];
            pc[u] = v < CX_HIST_BINS ? v : CX_HIST_BINS - 1;
            atomicAdd(&s_cur[pc[u]], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CX_HIST_BINS; i += CX_THREADS)
        if (s_cur[i]) s_cur[i] = atomicAdd(&cursor[i], s_cur[i]);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < CX_INDEX_PER_THREAD; u++) {
        const uint64_t j = j0 + (uint64_t)u * CX_THREADS;
        if (j < n_ov) index[atomicAdd(&s_cur[pc[u]], 1u)] = (uint32_t)j;
    }
}

}  // namespace

void compact_release(psk_ctx *ctx)
{
    dev_release(ctx->cx_slots);
    dev_release(ctx->cx_ov);
    dev_release(ctx->cx_ov_row);
    dev_release(ctx->cx_ov_pc);
    dev_release(ctx->cx_pc_index);
    ctx->cx_pc_hist.clear();
    ctx->cx_pc_start.clear();
    ctx->cx_valid = false;
    ctx->cx_n_ov = 0;
    ctx->cx_plan.valid = false;
}

int compact_encode(psk_ctx *ctx)
{
    ctx->cx_valid = false;
    ctx->cx_plan.valid = false;   // the scan plan belongs to the matrix and its encoded copy
    const uint64_t M = ctx->n_kmers;
    const int n = ctx->n_samples, wpr = ctx->wpr;
    const bool trace = env_flag("PSK_TRACE");
    if (n < CX_MIN_SAMPLES || n > CX_MAX_SAMPLES || M == 0 || M > 0xffffffffull || (wpr != 2 && wpr != 4)) {
        compact_release(ctx);
        return PSK_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t nb = div_up(M, CX_THREADS);
    PSK_TRY(dev_reserve(ctx, ctx->flags, std::max<uint64_t>(nb, 2 * CX_HIST_BINS) * 4));   // the counts, then the histogram and the buckets' cursors
    PSK_TRY(dev_reserve(ctx, ctx->misc, 64));
    uint32_t *cnt = ctx->flags.as<uint32_t>(), *d_total = ctx->misc.as<uint32_t>() + 6;
    const uint64_t *bits = ctx->bits.as<uint64_t>();
    cx_count_kernel<<<(unsigned)nb, CX_THREADS, 0, ctx->stream>>>(bits, M, wpr, n, cnt);
    PSK_HIP(ctx, hipGetLastError());
    PSK_TRY(dev_exclusive_scan_u32(ctx, cnt, cnt, nb, d_total));
    uint32_t n_ov = 0;
    PSK_HIP(ctx, hipMemcpyAsync(&n_ov, d_total, 4, hipMemcpyDeviceToHost, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double dense = (double)M * wpr * 8, enc = (double)M * 8 + (double)n_ov * (wpr * 8 + 4);
    if (enc > CX_MAX_SHARE * dense || (uint64_t)n_ov * CX_MAX_OVF_DIV > M) {
        compact_release(ctx);
        if (trace)
            fprintf(stderr, "[psk] compact rows: declined (%.3f of the dense bytes; %llu of %llu rows overflow)\n", enc / dense,
                    (unsigned long long)n_ov, (unsigned long long)M);
        return PSK_OK;
    }
    PSK_TRY(dev_reserve(ctx, ctx->cx_slots, (M + 1) / 2 * 16));
    PSK_TRY(dev_reserve(ctx, ctx->cx_ov, (n_ov ? n_ov : 1) * (uint64_t)wpr * 8));
    PSK_TRY(dev_reserve(ctx, ctx->cx_ov_row, (n_ov ? n_ov : 1) * 4ull));
    PSK_TRY(dev_reserve(ctx, ctx->cx_ov_pc, (n_ov ? n_ov : 1) * 2ull));
    PSK_TRY(dev_reserve(ctx, ctx->cx_pc_index, (n_ov ? n_ov : 1) * 4ull));
    cx_encode_kernel<<<(unsigned)nb, CX_THREADS, 0, ctx->stream>>>(bits, M, wpr, n, cnt, ctx->cx_slots.as<uint64_t>(),
                                                                  ctx->cx_ov.as<uint64_t>(), ctx->cx_ov_row.as<uint32_t>(),
                                                                  ctx->cx_ov_pc.as<uint16_t>());
    PSK_HIP(ctx, hipGetLastError());
    // the rows of each popcount, once per matrix (the encode kernel is done with the counts: same stream)
    uint32_t hist[CX_HIST_BINS];
    PSK_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(hist), ctx->stream));
    if (n_ov) {
        const uint64_t hb = std::min<uint64_t>(div_up(n_ov, CX_THREADS * 16), 1024);
        cx_pc_hist_kernel<<<(unsigned)hb, CX_THREADS, 0, ctx->stream>>>(ctx->cx_ov_pc.as<uint16_t>(), n_ov, cnt);
        PSK_HIP(ctx, hipGetLastError());
    }
    PSK_HIP(ctx, hipMemcpyAsync(hist, cnt, sizeof(hist), hipMemcpyDeviceToHost, ctx->stream));
    // the rows grouped by popcount, behind the histogram on the same stream: no host round trip of its own
    std::chrono::steady_clock::time_point t_idx;
    if (n_ov) {
        if (trace) {
            PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            t_idx = std::chrono::steady_clock::now();
        }
        uint32_t *cursor = cnt + CX_HIST_BINS;
        cx_pc_start_kernel<<<1, CX_THREADS, 0, ctx->stream>>>(cnt, cursor);
        PSK_HIP(ctx, hipGetLastError());
        cx_pc_index_kernel<<<(unsigned)div_up(n_ov, CX_INDEX_TILE), CX_THREADS, 0, ctx->stream>>>(ctx->cx_ov_pc.as<uint16_t>(), n_ov, cursor,
                                                                                                 ctx->cx_pc_index.as<uint32_t>());
        PSK_HIP(ctx, hipGetLastError());
    }
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (trace && n_ov)
        fprintf(stderr, "[psk] compact rows: index by popcount of %llu rows in %.3f ms\n", (unsigned long long)n_ov,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_idx).count());
    ctx->cx_pc_hist.assign(hist, hist + n + 1);
    ctx->cx_pc_start.assign(n + 2, 0);
    for (int pc = 0; pc <= n; pc++) ctx->cx_pc_start[pc + 1] = ctx->cx_pc_start[pc] + hist[pc];
    ctx->cx_n_ov = n_ov;
    ctx->cx_valid = true;
    if (trace) {
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[psk] compact rows: %.3f ms, %.1f MB of slots + %.1f MB of overflow rows (%llu of %llu) = %.3f of the dense bytes\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), M * 8 / 1e6,
                n_ov * (wpr * 8.0 + 4) / 1e6, (unsigned long long)n_ov, (unsigned long long)M, enc / dense);
        int lo = n + 1, hi = -1;
        for (int pc = 0; pc <= n; pc++)
            if (ctx->cx_pc_hist[pc]) { lo = std::min(lo, pc); hi = pc; }
        if (hi < 0) fprintf(stderr, "[psk] compact rows: no overflow row, empty popcount histogram\n");
        else fprintf(stderr, "[psk] compact rows: overflow rows have popcounts %d ... %d\n", lo, hi);
    }
    return PSK_OK;
}

extern "C" int psk_cx_pc_index(psk_ctx *ctx, uint32_t *index, uint64_t cap, uint64_t *pc_start, int n_start)
{
    if (!ctx) return PSK_EINVAL;
    if (!ctx->cx_valid) return psk_fail(ctx, PSK_ESTATE, "the matrix has no exception-coded copy");
    if (n_start < 0 || (size_t)n_start > ctx->cx_pc_start.size()) return psk_fail(ctx, PSK_EINVAL, "the index has %zu bucket starts", ctx->cx_pc_start.size());
    if (pc_start) std::copy(ctx->cx_pc_start.begin(), ctx->cx_pc_start.begin() + n_start, pc_start);
    if (index) {
        if (cap < ctx->cx_n_ov) return psk_fail(ctx, PSK_ERANGE, "buffer too small: %llu < %llu", (unsigned long long)cap, (unsigned long long)ctx->cx_n_ov);
        PSK_HIP(ctx, hipSetDevice(ctx->device));
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->cx_n_ov) PSK_HIP(ctx, hipMemcpy(index, ctx->cx_pc_index.p, ctx->cx_n_ov * 4, hipMemcpyDeviceToHost));
    }
    return PSK_OK;
}

extern "C" int psk_compact_info(const psk_ctx *ctx, int *encoded, uint64_t *overflow_rows)
{
    if (!ctx) return PSK_EINVAL;
    if (encoded) *encoded = ctx->cx_valid ? 1 : 0;
    if (overflow_rows) *overflow_rows = ctx->cx_valid ? ctx->cx_n_ov : 0;
    return PSK_OK;
}
