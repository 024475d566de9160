// The host's part of the k-mer assembly (`-a/--assembly`, asm.hip): strings of bases packed two bits a base, their reverse
// complement, the merge a + b[t:], the deduplicated list of a round, the bookkeeping of what has been emitted, the final order, the
// caps and the loop that ties the rounds together.  One round's matching -- every ordered pair's largest overlap, and which
// strings lie inside another -- is handed in as a function: asm.hip passes the device's, tests/asm_host_check.cpp a brute-force
// one.  Nothing here touches the device, a context or the environment (knob values arrive as arguments).
//
// The loop is the reference's kmer_assembler (modeling.py:1563-1605) with its set order replaced by a rule:
//   - a round's list is sorted by length, then lexicographically (A < C < G < T);
//   - a string in no pair of its round is emitted unless its reverse complement has been emitted before it; the round's
//     strings are offered in list order, so of a string and its reverse complement the earlier round's wins, and within a
//     round the lexicographically smaller;
//   - the next list is every a + b[t:], deduplicated, less the members that are a substring of a different member;
//   - the output is sorted by length, longest first, and lexicographically among equal lengths.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../../include/psk.h"

#ifdef __HIPCC__
#define ASM_HD __host__ __device__
#else
#define ASM_HD
#endif

// 32 bases per u64, the first base in the two most significant bits (a k-mer word of formats.kmer_to_word shifted up to the
// top), unused low bits of the last word zero: equal-length strings compare lexicographically word by word.
struct AsmStr {
    std::vector<uint64_t> w;
    uint32_t len = 0;
};

struct AsmPair {
    int32_t a, b, t;   // list positions; t = the overlap: suffix_t(a) == prefix_t(b)
};

ASM_HD inline uint32_t asm_words(uint32_t len) { return (len + 31u) >> 5; }

// the 32 bases of a packed string (nw words) from base `pos` on, zeros past its last word (seen by the kernels as well)
ASM_HD inline uint64_t asm_get32(const uint64_t *w, uint32_t nw, uint32_t pos)
{
    const uint32_t j = pos >> 5, r = (pos & 31u) * 2u;
    uint64_t x = j < nw ? w[j] << r : 0ull;
    if (r && j + 1 < nw) x |= w[j + 1] >> (64u - r);
    return x;
}

// the top `nb` (1..32) bases of a word
ASM_HD inline uint64_t asm_mask(uint32_t nb) { return nb >= 32u ? ~0ull : ~(~0ull >> (2u * nb)); }

// do the `count` bases of a from `s` on equal the first `count` bases of b?  (count <= |a| - s and count <= |b|)
ASM_HD inline bool asm_equal_at(const uint64_t *wa, uint32_t nwa, uint32_t s, const uint64_t *wb, uint32_t count)
{
    for (uint32_t c = 0; c < count; c += 32u) {
        const uint32_t nb = count - c < 32u ? count - c : 32u;
        if ((asm_get32(wa, nwa, s + c) ^ wb[c >> 5]) & asm_mask(nb)) return false;
    }
    return true;
}

inline int asm_code(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return -1;
    }
}

// false: a character that is no base
inline bool asm_pack(const char *s, size_t len, AsmStr *out)
{
    out->len = (uint32_t)len;
    out->w.assign(asm_words((uint32_t)len), 0);
    for (size_t i = 0; i < len; i++) {
        const int c = asm_code(s[i]);
        if (c < 0) return false;
        out->w[i >> 5] |= (uint64_t)c << (62 - 2 * (i & 31));
    }
    return true;
}

inline std::string asm_unpack(const AsmStr &s)
{
    std::string t(s.len, 'A');
    for (uint32_t i = 0; i < s.len; i++) t[i] = "ACGT"[(s.w[i >> 5] >> (62 - 2 * (i & 31))) & 3];
    return t;
}

// a k-mer in the package's encoding (2k bits, first base most significant)
inline AsmStr asm_from_kmer_word(uint64_t word, int k)
{
    AsmStr s;
    s.len = (uint32_t)k;
    s.w.assign(1, k >= 32 ? word : (word & ((1ull << (2 * k)) - 1)) << (64 - 2 * k));
    return s;
}

inline uint64_t asm_reverse_bases(uint64_t x)   // the 32 two-bit groups of a word in reverse order
{
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}

inline AsmStr asm_revcomp(const AsmStr &s)
{
    AsmStr r;
    r.len = s.len;
    const uint32_t nw = asm_words(s.len);
    r.w.assign(nw, 0);
    if (!nw) return r;
    std::vector<uint64_t> t(nw);   // the complement, words and bases reversed: the pad of the last word now leads
    for (uint32_t j = 0; j < nw; j++) t[j] = asm_reverse_bases(~s.w[nw - 1 - j]);
    const uint32_t sh = 64u * nw - 2u * s.len;   // 0..62 pad bits to shift out
    for (uint32_t j = 0; j < nw; j++) r.w[j] = sh ? (t[j] << sh) | (j + 1 < nw ? t[j + 1] >> (64u - sh) : 0ull) : t[j];
    return r;
}

// dst += src[from:]
inline void asm_append(AsmStr &dst, const AsmStr &src, uint32_t from)
{
    const uint32_t nws = asm_words(src.len);
    for (uint32_t pos = from; pos < src.len; pos += 32u) {
        const uint32_t nb = src.len - pos < 32u ? src.len - pos : 32u;
        const uint64_t chunk = asm_get32(src.w.data(), nws, pos) & asm_mask(nb);
        const uint32_t off = dst.len & 31u;
        if (off == 0) {
            dst.w.push_back(chunk);
        } else {
            dst.w.back() |= chunk >> (2u * off);
            if (nb > 32u - off) dst.w.push_back(chunk << (2u * (32u - off)));
        }
        dst.len += nb;
    }
}

// a + b[t:]
inline AsmStr asm_merge(const AsmStr &a, const AsmStr &b, uint32_t t)
{
    AsmStr m = a;
    asm_append(m, b, t);
    return m;
}

// the order of a round's list: by length, then lexicographically
struct AsmLess {
    bool operator()(const AsmStr &x, const AsmStr &y) const { return x.len != y.len ? x.len < y.len : x.w < y.w; }
};
inline bool asm_same(const AsmStr &x, const AsmStr &y) { return x.len == y.len && x.w == y.w; }

// sorted by AsmLess, exact duplicates dropped
inline void asm_sort_unique(std::vector<AsmStr> &list)
{
    std::sort(list.begin(), list.end(), AsmLess());
    list.erase(std::unique(list.begin(), list.end(), asm_same), list.end());
}

// the output's order: longest first, lexicographically among equal lengths
inline void asm_final_order(std::vector<AsmStr> &seqs)
{
    std::stable_sort(seqs.begin(), seqs.end(), [](const AsmStr &x, const AsmStr &y) { return x.len != y.len ? x.len > y.len : x.w < y.w; });
}

// What has been emitted (:1584-1587, :1601-1604): a string is refused when its reverse complement has been emitted; nothing else
// is looked at, as in the reference.
struct AsmEmitted {
    std::set<AsmStr, AsmLess> seen;
    std::vector<AsmStr> out;
    bool offer(const AsmStr &s)
    {
        if (seen.count(asm_revcomp(s))) return false;
        seen.insert(s);
        out.push_back(s);
        return true;
    }
};

// The limits of a run (PSK_ASM_MAX_STRINGS, PSK_ASM_MAX_PAIRS, PSK_ASM_MAX_LEN).  A list of exactly max_strings strings, a round
// of exactly max_pairs pairs and a string of exactly max_len bases pass; one more does not.
struct AsmCaps {
    int64_t max_strings = 1 << 20, max_pairs = 1 << 22, max_len = 65535;
};

inline std::string asm_text(const char *fmt, long long a, int b, long long c)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}

// "" when the list of `round` is within the caps, else the message
inline std::string asm_check_list(const std::vector<AsmStr> &list, const AsmCaps &caps, int round)
{
    if ((int64_t)list.size() > caps.max_strings)
        return asm_text("PSK_ASM_MAX_STRINGS=%lld: the list of round %d has %lld strings", caps.max_strings, round, (long long)list.size());
    for (const AsmStr &s : list)
        if ((int64_t)s.len > caps.max_len)
            return asm_text("PSK_ASM_MAX_LEN=%lld: a string of round %d has %lld bases", caps.max_len, round, (long long)s.len);
    return "";
}

inline std::string asm_check_pairs(uint64_t n_pairs, const AsmCaps &caps, int round)
{
    if (n_pairs > (uint64_t)caps.max_pairs)
        return asm_text("PSK_ASM_MAX_PAIRS=%lld: round %d has %lld overlapping pairs", caps.max_pairs, round, (long long)n_pairs);
    return "";
}

// the layout the matching takes: the words of all strings one after the other, where each starts, its length in bases
inline void asm_flatten(const std::vector<AsmStr> &list, std::vector<uint64_t> *words, std::vector<uint64_t> *word_off, std::vector<uint32_t> *len)
{
    words->clear();
    word_off->resize(list.size());
    len->resize(list.size());
    for (size_t i = 0; i < list.size(); i++) {
        (*word_off)[i] = words->size();
        (*len)[i] = list[i].len;
        words->insert(words->end(), list[i].w.begin(), list[i].w.end());
    }
}

// One round's matching over `list` with overlaps of at least min_olap bases: contained[i] != 0 where string i is a substring of
// a different string; the pairs among the strings that are NOT contained (positions in `list` as given), up to pair_cap of them
// in any order into *pairs, their true number into *n_pairs.  (A round's merged list holds many times the strings that survive
// string_set; the reference pairs the survivors only, :1596-1599, and so does the cap.)  PSK_OK; PSK_ERANGE when there are more
// than pair_cap pairs (*n_pairs is set); anything else is an error whose text is in *err.
typedef std::function<int(const std::vector<AsmStr> &list, int min_olap, uint64_t pair_cap, std::vector<AsmPair> *pairs, uint64_t *n_pairs,
                          std::vector<uint8_t> *contained, std::string *err)>
    AsmRoundFn;

struct AsmResult {
    std::vector<AsmStr> seqs;   // in the output's order
    int rounds = 0;             // rounds that merged something
};

// The whole loop over the k-mers of `list` (as given: the caller has appended the reverse complements when it wants both
// strands).  PSK_OK; PSK_ERANGE with the cap's message in *err; any other code is the matching's own.
inline int asm_assemble(std::vector<AsmStr> list, int k, const AsmCaps &caps, const AsmRoundFn &match, AsmResult *res, std::string *err)
{
    AsmEmitted emitted;
    res->rounds = 0;
    std::stable_sort(list.begin(), list.end(), AsmLess());   // round 0 keeps its duplicates (a palindrome and its reverse complement)
    std::vector<AsmPair> pairs;
    std::vector<uint8_t> contained;
    for (int round = 0; !list.empty(); round++) {
        *err = asm_check_list(list, caps, round);
        if (!err->empty()) return PSK_ERANGE;
        uint64_t n_pairs = 0;
        const int rc = match(list, k - 1, (uint64_t)caps.max_pairs, &pairs, &n_pairs, &contained, err);
        if (rc == PSK_ERANGE || (rc == PSK_OK && n_pairs > (uint64_t)caps.max_pairs)) {
            *err = asm_check_pairs(n_pairs, caps, round);
            return PSK_ERANGE;
        }
        if (rc != PSK_OK) return rc;
        // string_set (:1532-1535): the members inside a different member leave, and their pairs with them
        if (std::find_if(contained.begin(), contained.end(), [](uint8_t c) { return c != 0; }) != contained.end()) {
            std::vector<int32_t> to(list.size(), -1);
            std::vector<AsmStr> kept;
            for (size_t i = 0; i < list.size(); i++)
                if (!contained[i]) {
                    to[i] = (int32_t)kept.size();
                    kept.push_back(std::move(list[i]));
                }
            list.swap(kept);
            size_t n = 0;
            for (const AsmPair &p : pairs)
                if (to[p.a] >= 0 && to[p.b] >= 0) pairs[n++] = AsmPair{to[p.a], to[p.b], p.t};
            pairs.resize(n);
        }
        if (pairs.empty()) break;
        std::vector<uint8_t> in_pair(list.size(), 0);
        for (const AsmPair &p : pairs) in_pair[p.a] = in_pair[p.b] = 1;
        for (size_t i = 0; i < list.size(); i++)
            if (!in_pair[i]) emitted.offer(list[i]);
        std::vector<AsmStr> merged;
        merged.reserve(pairs.size());
        for (const AsmPair &p : pairs) {
            const int64_t len = (int64_t)list[p.a].len + list[p.b].len - p.t;
            if (len > caps.max_len) {   // before the string is built: a repeat doubles its strings every round
                *err = asm_text("PSK_ASM_MAX_LEN=%lld: a string of round %d has %lld bases", caps.max_len, round + 1, (long long)len);
                return PSK_ERANGE;
            }
            merged.push_back(asm_merge(list[p.a], list[p.b], (uint32_t)p.t));
        }
        asm_sort_unique(merged);
        list.swap(merged);
        res->rounds++;
    }
    for (const AsmStr &s : list) emitted.offer(s);
    res->seqs.swap(emitted.out);
    asm_final_order(res->seqs);
    return PSK_OK;
}
