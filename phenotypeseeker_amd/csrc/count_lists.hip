// a1: the list entry points -- a sample's list to the host, split points of the sorted lists, ranges copied device to
// device, lists set from device arrays, and the count lookups of modeling.py:324-329.
#include "psk_internal.h"

namespace {

// binary search of `n` query words in a sorted list; 0 if absent
__global__ void lookup_counts_kernel(const uint64_t *__restrict__ words, const uint32_t *__restrict__ freqs,
                                     uint64_t nu, const uint64_t *__restrict__ q, uint64_t n,
                                     uint32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = q[i];
    uint64_t lo = 0, hi = nu;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (words[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[i] = (lo < nu && words[lo] == key) ? freqs[lo] : 0u;
}

}  // namespace

extern "C" int psk_get_list(psk_ctx *ctx, int sample_idx, uint64_t *words, uint32_t *freqs, uint64_t cap)
{
    if (!ctx) return PSK_EINVAL;
    if (sample_idx < 0 || sample_idx >= ctx->n_samples || !ctx->lists[sample_idx].done)
        return psk_fail(ctx, PSK_ESTATE, "sample %d has not been counted", sample_idx);
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    PSK_TRY(dense_materialize(ctx, sample_idx, 1));
    const SampleList &L = ctx->lists[sample_idx];
    if (cap < L.n_unique) return psk_fail(ctx, PSK_ERANGE, "buffer too small: %llu < %llu", (unsigned long long)cap,
                                          (unsigned long long)L.n_unique);
    if (L.n_unique) {
        if (words) PSK_HIP(ctx, hipMemcpy(words, L.words, L.n_unique * 8, hipMemcpyDeviceToHost));
        if (freqs) PSK_HIP(ctx, hipMemcpy(freqs, L.freqs, L.n_unique * 4, hipMemcpyDeviceToHost));
    }
    return PSK_OK;
}

namespace {

// thread (i, b): lower bound of bounds[b] in the sorted list of sample i
struct SplitRef { const uint64_t *words; uint64_t n; };
__global__ void lists_split_kernel(const SplitRef *__restrict__ refs, int n, const uint64_t *__restrict__ bounds, int n_bounds,
                                   uint64_t *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_bounds) return;
    const int i = t / n_bounds, b = t % n_bounds;
    const uint64_t key = bounds[b];
    uint64_t lo = 0, hi = refs[i].n;
    if (b > 0 && key == 0) lo = hi;  // "end of the word space"
    const uint64_t *w = refs[i].words;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (w[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[t] = lo;
}

// 1 when words[0 .. n) ascend strictly and stay inside [lo, hi) (hi == 0: unbounded)
__global__ void list_check_kernel(const uint64_t *__restrict__ words, uint64_t n, uint64_t lo, uint64_t hi, uint32_t *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t w = words[i];
    if ((i > 0 && words[i - 1] >= w) || w < lo || (hi && w >= hi)) atomicOr(bad, 1u);
}

}  // namespace

extern "C" int psk_lists_split(psk_ctx *ctx, int first_sample_idx, int n, const uint64_t *bounds, int n_bounds,
                               uint64_t *offsets_out)
{
    if (!ctx) return PSK_EINVAL;
    if (n < 0 || first_sample_idx < 0 || first_sample_idx + n > ctx->n_samples)
        return psk_fail(ctx, PSK_EINVAL, "sample range out of bounds");
    if (n == 0 || n_bounds == 0) return PSK_OK;
    if (!bounds || !offsets_out || n_bounds < 0) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    std::vector<SplitRef> refs(n);
    for (int i = 0; i < n; i++)
        if (!ctx->lists[first_sample_idx + i].done)
            return psk_fail(ctx, PSK_ESTATE, "sample %d has not been counted", first_sample_idx + i);
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    PSK_TRY(dense_materialize(ctx, first_sample_idx, n));
    for (int i = 0; i < n; i++) {
        const SampleList &L = ctx->lists[first_sample_idx + i];
        refs[i].words = L.words;
        refs[i].n = L.n_unique;
    }
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * n_bounds;
    const size_t b_refs = (size_t)n * sizeof(SplitRef), b_bounds = (size_t)n_bounds * 8;
    PSK_TRY(dev_reserve(ctx, ctx->flags, b_refs + b_bounds + cells * 8));
    uint8_t *base = ctx->flags.as<uint8_t>();
    PSK_HIP(ctx, hipMemcpyAsync(base, refs.data(), b_refs, hipMemcpyHostToDevice, ctx->stream));
    PSK_HIP(ctx, hipMemcpyAsync(base + b_refs, bounds, b_bounds, hipMemcpyHostToDevice, ctx->stream));
    uint64_t *d_out = reinterpret_cast<uint64_t *>(base + b_refs + b_bounds);
    lists_split_kernel<<<div_up(cells, 256), 256, 0, ctx->stream>>>(reinterpret_cast<const SplitRef *>(base), n,
                                                                  reinterpret_cast<const uint64_t *>(base + b_refs), n_bounds, d_out);
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipMemcpyAsync(offsets_out, d_out, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

extern "C" int psk_copy_list_ranges(psk_ctx *ctx, int n_ranges, const int32_t *sample_idx, const uint64_t *start,
                                    const uint64_t *count, void *device_words_dst, void *device_freqs_dst)
{
    if (!ctx) return PSK_EINVAL;
    if (n_ranges < 0) return psk_fail(ctx, PSK_EINVAL, "negative range count");
    if (n_ranges == 0) return PSK_OK;
    if (!sample_idx || !start || !count) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    uint64_t total = 0;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    for (int r = 0; r < n_ranges; r++) {
        const int si = sample_idx[r];
        if (si < 0 || si >= ctx->n_samples || !ctx->lists[si].done)
            return psk_fail(ctx, PSK_ESTATE, "sample %d has not been counted", si);
        PSK_TRY(dense_materialize(ctx, si, 1));
        const SampleList &L = ctx->lists[si];
        if (start[r] > L.n_unique || count[r] > L.n_unique - start[r])
            return psk_fail(ctx, PSK_ERANGE, "range %d lies outside the list of sample %d", r, si);
        total += count[r];
    }
    if (total == 0) return PSK_OK;
    if (!device_words_dst || !device_freqs_dst) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t *dw = static_cast<uint64_t *>(device_words_dst);
    uint32_t *df = static_cast<uint32_t *>(device_freqs_dst);
    for (int r = 0; r < n_ranges; r++) {
        if (count[r] == 0) continue;
        const SampleList &L = ctx->lists[sample_idx[r]];
        PSK_HIP(ctx, hipMemcpyAsync(dw, L.words + start[r], count[r] * 8, hipMemcpyDeviceToDevice, ctx->stream));
        PSK_HIP(ctx, hipMemcpyAsync(df, L.freqs + start[r], count[r] * 4, hipMemcpyDeviceToDevice, ctx->stream));
        dw += count[r];
        df += count[r];
    }
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}

extern "C" int psk_release_lists(psk_ctx *ctx)
{
    if (!ctx) return PSK_EINVAL;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t st : {ctx->copy_stream, ctx->copy_more[0], ctx->copy_more[1], ctx->copy_more[2], ctx->frame_stream, ctx->sketch_stream})
        if (st) PSK_HIP(ctx, hipStreamSynchronize(st));
    reset_lists(ctx, ctx->n_samples);   // every sample is "not counted" again
    arena_release(ctx);                 // and the chunks go back to the device, not to the next run
    ctx->have_presence = false;
    return PSK_OK;
}

extern "C" int psk_set_lists_device(psk_ctx *ctx, int n_lists, const int32_t *sample_idx, const uint64_t *count,
                                    const uint64_t *n_total, const void *device_words, const void *device_freqs)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->k == 0) return psk_fail(ctx, PSK_ESTATE, "psk_begin has not been called");
    if (n_lists < 0) return psk_fail(ctx, PSK_EINVAL, "negative list count");
    if (n_lists == 0) return PSK_OK;
    if (!sample_idx || !count) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    uint64_t total = 0;
    for (int r = 0; r < n_lists; r++) {
        if (sample_idx[r] < 0 || sample_idx[r] >= ctx->n_samples) return psk_fail(ctx, PSK_EINVAL, "sample index out of range");
        if (count[r] >= (1ull << 32)) return psk_fail(ctx, PSK_ERANGE, "list with more than 2^32 entries");
        total += count[r];
    }
    if (total && (!device_words || !device_freqs)) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->have_presence = false;
    PSK_TRY(dev_reserve(ctx, ctx->misc, 64));
    uint32_t *bad = ctx->misc.as<uint32_t>() + 12;
    PSK_HIP(ctx, hipMemsetAsync(bad, 0, 4, ctx->stream));
    const uint64_t *sw = static_cast<const uint64_t *>(device_words);
    const uint32_t *sf = static_cast<const uint32_t *>(device_freqs);
    for (int r = 0; r < n_lists; r++) {
        SampleList &S = ctx->lists[sample_idx[r]];
        S = SampleList();
        const uint64_t n = count[r];
        if (n) {
            list_check_kernel<<<div_up(n, 256), 256, 0, ctx->stream>>>(sw, n, ctx->slab_lo, ctx->slab_hi, bad);
            PSK_HIP(ctx, hipGetLastError());
            PSK_TRY(arena_alloc(ctx, n * 8, (void **)&S.words));
            PSK_TRY(arena_alloc(ctx, n * 4, (void **)&S.freqs));
            PSK_HIP(ctx, hipMemcpyAsync(S.words, sw, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
            PSK_HIP(ctx, hipMemcpyAsync(S.freqs, sf, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
            sw += n;
            sf += n;
        }
        S.n_unique = n;
        S.n_total = n_total ? n_total[r] : 0;
        S.done = true;
    }
    uint32_t h_bad = 0;
    PSK_HIP(ctx, hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_bad) {
        for (int r = 0; r < n_lists; r++) ctx->lists[sample_idx[r]] = SampleList();
        return psk_fail(ctx, PSK_EINVAL, "a list does not ascend inside the context's slab");
    }
    return PSK_OK;
}

extern "C" int psk_lookup_counts(psk_ctx *ctx, int sample_idx, const uint64_t *words, uint64_t n, uint32_t *freqs)
{
    if (!ctx) return PSK_EINVAL;
    if (sample_idx < 0 || sample_idx >= ctx->n_samples || !ctx->lists[sample_idx].done)
        return psk_fail(ctx, PSK_ESTATE, "sample %d has not been counted", sample_idx);
    if (n == 0) return PSK_OK;
    if (!words || !freqs) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    const SampleList &L = ctx->lists[sample_idx];
    PSK_TRY(dev_reserve(ctx, ctx->flags, n * 8));
    PSK_TRY(dev_reserve(ctx, ctx->starts, n * 4));
    PSK_HIP(ctx, hipMemcpyAsync(ctx->flags.p, words, n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (L.dense && !L.words)
        PSK_TRY(dense_lookup_counts(ctx, L, ctx->flags.as<uint64_t>(), n, ctx->starts.as<uint32_t>()));
    else
        lookup_counts_kernel<<<div_up(n, 256), 256, 0, ctx->stream>>>(L.words, L.freqs, L.n_unique, ctx->flags.as<uint64_t>(),
                                                                      n, ctx->starts.as<uint32_t>());
    PSK_HIP(ctx, hipGetLastError());
    PSK_HIP(ctx, hipMemcpyAsync(freqs, ctx->starts.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PSK_OK;
}
