// `-a/--assembly`: the reference's kmer_assembler (modeling.py:1526-1605) with every round's all-pairs string matching on the
// device.  The reference compares every ordered pair of a round's strings in Python (quadratic in --n_kmers in the first round,
// exponential in the number of branch points afterwards); here a round is
//   asm_key_kernel       key of a string = its first m = min_olap bases (m <= 31: one u64), payload = its list position
//   radix sort           of the (key, position) pairs (radix_sort.hip)
//   asm_contained_kernel \ one work item per (string a, start s <= |a| - m): the m-base window of a at s is looked up in the
//   asm_match_kernel     / sorted keys by binary search, and every string b of the bucket (b at another list position) is
//                        compared with a[s:] over their min(|a| - s, |b|) common bases, word by word with unaligned shifts.
//                        Equal and |b| <= |a| - s and b is another string than a: b lies inside a, and the first kernel sets
//                        contained[b].  Equal and |a| - s <= |b|: a[s:] is a prefix of b, an overlap of t = |a| - s; the
//                        pair's overlap is its largest t, so the second kernel reports the pair from this item only when no
//                        smaller start of a matches b as well.
// The loop's rounds drop the contained strings before they pair the rest (string_set, :1532-1535, then pick_overlaps), and a
// round's merged list holds many more strings than survive -- 5,000 against 100 in the two-bubble golden case --, so the match
// kernel takes the flags of the first as a mask: pairs are formed among the unmasked strings only.  psk_asm_round passes no mask.
// Pairs are appended with one global atomic per workgroup and trip: every thread counts its pairs, the workgroup scans the
// counts, one thread reserves the workgroup's range, and the threads that had any walk their bucket again and write.  The
// counter keeps counting past pair_cap (nothing is written there), so the caller learns the true number.  No workgroup waits
// for another.  The host's part of the loop is asm_host.h.
//
// Launch shape: 256 threads, one work item per thread and trip, min(items / 256, CUs x 8) workgroups (PSK_GRID_MULT replaces the
// 8) striding over the items: integer kernels bound by the latency of their dependent loads, so they want many waves per CU.
// The shape has not been varied: docs/NOTEBOOK.md, Round 29, has the first times of whole calls and nothing else.
#include "asm_host.h"
#include "dev_utils.h"
#include "psk_internal.h"
#include "solver_host.h"

namespace {

constexpr int AS_THREADS = 256;

__global__ __launch_bounds__(AS_THREADS) void asm_key_kernel(const uint64_t *__restrict__ words, const uint64_t *__restrict__ word_off,
                                                             const uint32_t *__restrict__ len, uint32_t n, uint32_t m,
                                                             uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * AS_THREADS + threadIdx.x;
    if (i >= n) return;
    keys[i] = asm_get32(words + word_off[i], asm_words(len[i]), 0) >> (64u - 2u * m);
    vals[i] = i;
}

struct AsmLists {
    const uint64_t *words, *word_off;   // word_off[n]
    const uint32_t *len;                // len[n], every one >= m
    const uint64_t *item_off;           // item_off[n + 1]: exclusive prefix of |a| - m + 1
    const uint64_t *keys;               // keys[n], ascending
    const uint32_t *idx;                // idx[n]: list position of the string with keys[i]
    uint32_t n, m;
};

// work item -> (a, s): the string whose items hold `item` is the last a with item_off[a] <= item
__device__ __forceinline__ void asm_item(const AsmLists &L, uint64_t item, uint32_t *a, uint32_t *s)
{
    uint32_t lo = 0, hi = L.n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (L.item_off[mid] <= item) lo = mid;
        else hi = mid;
    }
    *a = lo;
    *s = (uint32_t)(item - L.item_off[lo]);
}

enum { AS_CONTAINED = 0, AS_COUNT = 1, AS_WRITE = 2 };

// Work item (a, s) against its bucket.  AS_CONTAINED: sets contained[b] for the b inside a at s.  AS_COUNT / AS_WRITE: the pairs
// (a, b) whose overlap starts at s, b not masked; AS_WRITE puts them into slots `slot`, `slot` + 1, ... below pair_cap.
template <int MODE>
__device__ __forceinline__ uint32_t asm_walk(const AsmLists &L, uint32_t a, uint32_t s, const uint32_t *__restrict__ mask, uint64_t slot, uint64_t pair_cap,
                                             int32_t *__restrict__ pairs, uint32_t *__restrict__ contained)
{
    const uint32_t la = L.len[a], nwa = asm_words(la), rem = la - s;
    const uint64_t *wa = L.words + L.word_off[a];
    const uint64_t key = asm_get32(wa, nwa, s) >> (64u - 2u * L.m);
    uint32_t lo = 0, hi = L.n;   // first sorted key >= key
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (L.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    uint32_t found = 0;
    for (uint32_t i = lo; i < L.n && L.keys[i] == key; i++) {
        const uint32_t b = L.idx[i];
        if (b == a) continue;
        const uint32_t lb = L.len[b];
        if (MODE == AS_CONTAINED ? lb > rem || (s == 0 && lb == la) : rem > lb || (mask && mask[b])) continue;
        const uint64_t *wb = L.words + L.word_off[b];
        if (!asm_equal_at(wa, nwa, s, wb, rem < lb ? rem : lb)) continue;
        if (MODE == AS_CONTAINED) {
            contained[b] = 1u;   // (the same value from every thread that stores it; s == 0 and equal lengths: the same string, not a containment)
            continue;
        }
        // a[s:] is a prefix of b.  The pair's overlap is its largest: is there a start before s that matches b as well?
        bool earlier = false;
        for (uint32_t s2 = la > lb ? la - lb : 0; s2 < s && !earlier; s2++)
            earlier = (asm_get32(wa, nwa, s2) >> (64u - 2u * L.m)) == key && asm_equal_at(wa, nwa, s2, wb, la - s2);
        if (earlier) continue;
        if (MODE == AS_WRITE && slot + found < pair_cap) {
            int32_t *p = pairs + 3 * (slot + found);
            p[0] = (int32_t)a;
            p[1] = (int32_t)b;
            p[2] = (int32_t)rem;
        }
        found++;
    }
    return found;
}

__global__ __launch_bounds__(AS_THREADS) void asm_contained_kernel(AsmLists L, uint64_t total_items, uint32_t *__restrict__ contained)
{
    for (uint64_t item = (uint64_t)blockIdx.x * AS_THREADS + threadIdx.x; item < total_items; item += (uint64_t)gridDim.x * AS_THREADS) {
        uint32_t a, s;
        asm_item(L, item, &a, &s);
        asm_walk<AS_CONTAINED>(L, a, s, nullptr, 0, 0, nullptr, contained);
    }
}

// mask: null, or mask[i] != 0 takes string i out of the pairing (the contained strings of the loop's rounds)
__global__ __launch_bounds__(AS_THREADS) void asm_match_kernel(AsmLists L, uint64_t total_items, const uint32_t *__restrict__ mask, uint64_t pair_cap,
                                                               int32_t *__restrict__ pairs, unsigned long long *__restrict__ n_pairs)
{
    __shared__ uint32_t scan_lds[AS_THREADS / 64];
    __shared__ unsigned long long wg_base;
    // (the trip count is the workgroup's, not the thread's: every thread reaches the barriers of the scan)
    for (uint64_t base = (uint64_t)blockIdx.x * AS_THREADS; base < total_items; base += (uint64_t)gridDim.x * AS_THREADS) {
        const uint64_t item = base + threadIdx.x;
        uint32_t a = 0, s = 0, count = 0;
        if (item < total_items) {
            asm_item(L, item, &a, &s);
            if (!(mask && mask[a])) count = asm_walk<AS_COUNT>(L, a, s, mask, 0, 0, nullptr, nullptr);
        }
        uint32_t total;
        const uint32_t before = psk_block_excl_scan_u32<AS_THREADS>(count, &total, scan_lds);
        if (total == 0) continue;   // (the same in every thread)
        if (threadIdx.x == 0) wg_base = atomicAdd(n_pairs, (unsigned long long)total);
        __syncthreads();
        if (count) asm_walk<AS_WRITE>(L, a, s, mask, (uint64_t)wg_base + before, pair_cap, pairs, nullptr);
        __syncthreads();   // wg_base is rewritten in the next trip
    }
}

// One round on the device; the lists are the caller's host arrays (checked by the caller: n >= 1, 1 <= m <= 31, every length
// >= m).  drop_contained: pairs among the strings that are not contained only (the loop); else among all (psk_asm_round).
int asm_round_device(psk_ctx *ctx, const uint64_t *words, uint64_t n_words, const uint64_t *word_off, const uint32_t *len, uint32_t n, uint32_t m,
                     bool drop_contained, uint64_t pair_cap, int32_t *pairs_out, uint64_t *n_pairs_out, uint8_t *contained_out)
{
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> item_off((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) item_off[i + 1] = item_off[i] + (len[i] - m + 1);
    const uint64_t total_items = item_off[n];
    FitArr<uint64_t> d_words, d_off, d_items, d_keys_a, d_keys_b;
    FitArr<uint32_t> d_len, d_vals_a, d_vals_b, d_contained;
    FitArr<int32_t> d_pairs;
    FitArr<unsigned long long> d_n_pairs;
    PSK_HIP(ctx, d_words.upload(words, n_words, ctx->stream));
    PSK_HIP(ctx, d_off.upload(word_off, n, ctx->stream));
    PSK_HIP(ctx, d_len.upload(len, n, ctx->stream));
    PSK_HIP(ctx, d_items.upload(item_off, ctx->stream));
    PSK_HIP(ctx, d_keys_a.alloc(n));
    PSK_HIP(ctx, d_keys_b.alloc(n));
    PSK_HIP(ctx, d_vals_a.alloc(n));
    PSK_HIP(ctx, d_vals_b.alloc(n));
    PSK_HIP(ctx, d_contained.alloc(n));
    PSK_HIP(ctx, d_pairs.alloc((size_t)pair_cap * 3));
    PSK_HIP(ctx, d_n_pairs.alloc(1));
    PSK_HIP(ctx, d_contained.zero(ctx->stream));
    PSK_HIP(ctx, d_n_pairs.zero(ctx->stream));
    asm_key_kernel<<<div_up(n, AS_THREADS), AS_THREADS, 0, ctx->stream>>>(d_words, d_off, d_len, n, m, d_keys_a, d_vals_a);
    PSK_HIP(ctx, hipGetLastError());
    uint64_t *keys = nullptr;
    uint32_t *idx = nullptr;
    PSK_TRY(dev_radix_sort_kv(ctx, d_keys_a, d_keys_b, d_vals_a, d_vals_b, n, 0, 2 * (int)m, &keys, &idx));
    const AsmLists L = {d_words, d_off, d_len, d_items, keys, idx, n, m};
    const uint64_t grid_cap = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * (ctx->grid_mult ? ctx->grid_mult : 8);
    const uint64_t want = (total_items + AS_THREADS - 1) / AS_THREADS;
    const unsigned grid = (unsigned)(want < grid_cap ? want : grid_cap);
    asm_contained_kernel<<<grid, AS_THREADS, 0, ctx->stream>>>(L, total_items, d_contained);
    PSK_HIP(ctx, hipGetLastError());
    const uint32_t *mask = drop_contained ? (const uint32_t *)d_contained : nullptr;   // (the same stream: the flags are complete when the pairing starts)
    asm_match_kernel<<<grid, AS_THREADS, 0, ctx->stream>>>(L, total_items, mask, pair_cap, d_pairs, d_n_pairs);
    PSK_HIP(ctx, hipGetLastError());
    unsigned long long n_pairs = 0;
    std::vector<uint32_t> contained(n);
    PSK_HIP(ctx, d_n_pairs.download(&n_pairs, 1, ctx->stream));
    PSK_HIP(ctx, d_contained.download(contained.data(), n, ctx->stream));
    PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_pairs_out = n_pairs;
    for (uint32_t i = 0; i < n; i++) contained_out[i] = contained[i] ? 1 : 0;
    const uint64_t have = n_pairs < pair_cap ? n_pairs : pair_cap;
    if (have) {
        PSK_HIP(ctx, d_pairs.download(pairs_out, (size_t)have * 3, ctx->stream));
        PSK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n_pairs > pair_cap)
        return psk_fail(ctx, PSK_ERANGE, "pair_cap=%llu: the list has %llu overlapping pairs", (unsigned long long)pair_cap, n_pairs);
    return PSK_OK;
}

constexpr int64_t ASM_KNOB_MAX_STRINGS = 1 << 24, ASM_KNOB_MAX_PAIRS = 1 << 28, ASM_KNOB_MAX_LEN = 1 << 24;

int check_round_args(psk_ctx *ctx, const uint64_t *word_off, const uint32_t *len, int64_t n, int min_olap, uint64_t *n_words)
{
    if (min_olap < 1 || min_olap > 31) return psk_fail(ctx, PSK_EINVAL, "min_olap must be 1..31 (k - 1 with k <= 32), got %d", min_olap);
    if (n > ASM_KNOB_MAX_STRINGS) return psk_fail(ctx, PSK_ERANGE, "%lld strings exceed the limit of %lld", (long long)n, (long long)ASM_KNOB_MAX_STRINGS);
    *n_words = 0;
    for (int64_t i = 0; i < n; i++) {
        if (len[i] < (uint32_t)min_olap || len[i] > (uint32_t)ASM_KNOB_MAX_LEN)
            return psk_fail(ctx, PSK_EINVAL, "string %lld has %u bases: expected %d..%lld", (long long)i, len[i], min_olap, (long long)ASM_KNOB_MAX_LEN);
        *n_words = std::max(*n_words, word_off[i] + asm_words(len[i]));
    }
    return PSK_OK;
}

}  // namespace

extern "C" int psk_asm_round(psk_ctx *ctx, const uint64_t *words, const uint64_t *word_off, const uint32_t *len_bases, int64_t n, int min_olap,
                             uint64_t pair_cap, int32_t *pairs_out, uint64_t *n_pairs_out, uint8_t *contained_out)
{
    if (!ctx) return PSK_EINVAL;
    if (n < 0 || !n_pairs_out || (n > 0 && (!words || !word_off || !len_bases || !contained_out)) || (pair_cap > 0 && !pairs_out))
        return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (pair_cap > (uint64_t)ASM_KNOB_MAX_PAIRS) return psk_fail(ctx, PSK_EINVAL, "pair_cap must be at most %lld", (long long)ASM_KNOB_MAX_PAIRS);
    *n_pairs_out = 0;
    uint64_t n_words = 0;
    PSK_TRY(check_round_args(ctx, word_off, len_bases, n, min_olap, &n_words));
    if (n == 0) return PSK_OK;
    return asm_round_device(ctx, words, n_words, word_off, len_bases, (uint32_t)n, (uint32_t)min_olap, false, pair_cap, pairs_out, n_pairs_out, contained_out);
}

extern "C" int psk_assemble(psk_ctx *ctx, const uint64_t *kmer_words, int64_t n, int k, int both_strands, char *text_out, uint64_t text_cap,
                            int64_t *n_seqs_out, uint64_t *text_len_out, int32_t *rounds_out)
{
    if (!ctx) return PSK_EINVAL;
    if (n < 0 || (n > 0 && !kmer_words) || !n_seqs_out || !text_len_out || (text_cap > 0 && !text_out)) return psk_fail(ctx, PSK_EINVAL, "null buffer");
    if (k < 2 || k > 32) return psk_fail(ctx, PSK_EINVAL, "k-mer length must be 2..32, got %d", k);
    AsmCaps caps;
    PSK_TRY(env_int(ctx, "PSK_ASM_MAX_STRINGS", 1, ASM_KNOB_MAX_STRINGS, &caps.max_strings));
    PSK_TRY(env_int(ctx, "PSK_ASM_MAX_PAIRS", 1, ASM_KNOB_MAX_PAIRS, &caps.max_pairs));
    PSK_TRY(env_int(ctx, "PSK_ASM_MAX_LEN", 1, ASM_KNOB_MAX_LEN, &caps.max_len));
    *n_seqs_out = 0;
    *text_len_out = 0;
    if (rounds_out) *rounds_out = 0;
    std::vector<AsmStr> list;
    list.reserve((size_t)n * (both_strands ? 2 : 1));
    for (int64_t i = 0; i < n; i++) list.push_back(asm_from_kmer_word(kmer_words[i], k));
    if (both_strands)
        for (int64_t i = 0; i < n; i++) list.push_back(asm_revcomp(list[(size_t)i]));
    std::vector<uint64_t> words, word_off;
    std::vector<uint32_t> len;
    std::vector<int32_t> triples;
    const AsmRoundFn match = [&](const std::vector<AsmStr> &cur, int min_olap, uint64_t pair_cap, std::vector<AsmPair> *pairs, uint64_t *n_pairs,
                                 std::vector<uint8_t> *contained, std::string *err) {
        asm_flatten(cur, &words, &word_off, &len);
        // a round of n strings has at most n (n - 1) pairs: the buffer need not be larger
        const uint64_t all = (uint64_t)cur.size() * (cur.size() - 1);
        const uint64_t cap = all < pair_cap ? all : pair_cap;
        triples.resize((size_t)cap * 3);
        contained->assign(cur.size(), 0);
        const int rc = asm_round_device(ctx, words.data(), words.size(), word_off.data(), len.data(), (uint32_t)cur.size(), (uint32_t)min_olap, true, cap,
                                        triples.data(), n_pairs, contained->data());
        if (rc != PSK_OK) {
            *err = psk_error_text(ctx);
            return rc;
        }
        pairs->resize((size_t)*n_pairs);
        for (size_t i = 0; i < pairs->size(); i++) (*pairs)[i] = AsmPair{triples[3 * i], triples[3 * i + 1], triples[3 * i + 2]};
        return (int)PSK_OK;
    };
    AsmResult res;
    std::string err;
    const int rc = asm_assemble(std::move(list), k, caps, match, &res, &err);
    if (rc != PSK_OK) return psk_fail(ctx, rc, "%s", err.c_str());
    uint64_t need = 0;
    for (const AsmStr &s : res.seqs) need += s.len + 1;
    if (need) need--;   // newlines BETWEEN the sequences
    *n_seqs_out = (int64_t)res.seqs.size();
    *text_len_out = need;
    if (rounds_out) *rounds_out = res.rounds;
    if (need > text_cap) return psk_fail(ctx, PSK_ERANGE, "text_cap=%llu: the sequences take %llu bytes", (unsigned long long)text_cap, (unsigned long long)need);
    uint64_t at = 0;
    for (size_t i = 0; i < res.seqs.size(); i++) {
        if (i) text_out[at++] = '\n';
        const std::string t = asm_unpack(res.seqs[i]);
        memcpy(text_out + at, t.data(), t.size());
        at += t.size();
    }
    return PSK_OK;
}
