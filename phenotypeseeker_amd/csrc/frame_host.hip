// a1, host half: record framing only (headers, FASTQ separator/quality lines, control bytes) -> clean stream: bases + '\n'
// window breaks.  No device code: the GPU's framing is frame_gpu.hip, the counting chain count_chain.hip.
#include "kmer_windows.h"   // EX_SEG: the padding the extract kernel wants
#include "psk_internal.h"

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

// ------------------------------------------------------------------------------------------------
// Host framing.  Tokeniser contract of glistmaker 4.2.3 as established by probing the binary
// (DESIGN.md "Tokeniser contract"; fixtures tests/golden/tokenizer_cases.json).
// ------------------------------------------------------------------------------------------------
namespace {
enum { ST_INIT, ST_FA_HDR, ST_FA_SEQ, ST_FQ_HDR, ST_FQ_SEQ, ST_FQ_PLUS, ST_FQ_QUAL, ST_FQ_H, ST_FQ_HSKIP };
enum { CL_BREAK = 0, CL_BASE = 1, CL_SKIP = 2 };

struct ClassTable {
    uint8_t t[256];
    ClassTable()
    {
        for (int c = 0; c < 256; c++) t[c] = (c < 32) ? CL_SKIP : CL_BREAK;
        for (const char *p = "ACGTUacgtu"; *p; p++) t[(unsigned char)*p] = CL_BASE;
    }
};
const ClassTable g_cls;

static inline bool is_base_byte(uint8_t c)
{
    const uint8_t x = c | 0x20;  // fold case
    return (x == 'a') | (x == 'c') | (x == 'g') | (x == 't') | (x == 'u');
}

// length of the leading run of base bytes of p[0..n): 16 bytes per step on the host's SSE2 unit
static inline size_t base_run_length(const uint8_t *p, size_t n)
{
    size_t j = 0;
#if defined(__SSE2__)
    const __m128i fold = _mm_set1_epi8(0x20);
    const __m128i ca = _mm_set1_epi8('a'), cc = _mm_set1_epi8('c'), cg = _mm_set1_epi8('g'), ct = _mm_set1_epi8('t'),
                  cu = _mm_set1_epi8('u');
    while (j + 16 <= n) {
        const __m128i v = _mm_or_si128(_mm_loadu_si128(reinterpret_cast<const __m128i *>(p + j)), fold);
        const __m128i ok = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(v, ca), _mm_cmpeq_epi8(v, cc)),
                                        _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(v, cg), _mm_cmpeq_epi8(v, ct)),
                                                     _mm_cmpeq_epi8(v, cu)));
        const unsigned m = (unsigned)_mm_movemask_epi8(ok);
        if (m != 0xffffu) return j + (size_t)__builtin_ctz(~m);
        j += 16;
    }
#endif
    while (j < n && is_base_byte(p[j])) j++;
    return j;
}
}  // namespace

// k > 0: *n_windows receives the number of k-base windows of the clean stream (sum over its runs of
// max(0, run - k + 1)), i.e. the number of words the extract kernel emits when no slab filter is set.
static int64_t frame_sequence_counting(const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap, int k,
                                       uint64_t *n_windows)
{
    size_t o = 0;
    int st = ST_INIT;
    bool last_break = true;  // collapse runs of breaks; no leading break needed
    size_t run_start = 0;    // output offset where the current run of bases began
    uint64_t wins = 0;
    auto close_run = [&]() {
        const size_t run = o - run_start;
        if (k > 0 && run >= (size_t)k) wins += run - (size_t)k + 1;
    };
    auto put_break = [&]() {
        if (!last_break) { close_run(); out[o++] = '\n'; last_break = true; run_start = o; }
    };
    auto finish = [&]() -> int64_t {
        if (!last_break) close_run();
        if (n_windows) *n_windows = wins;
        return (int64_t)o;
    };
    if (out_cap < len) return PSK_ERANGE;
    for (size_t i = 0; i < len; i++) {
        const uint8_t c = bytes[i];
        if (c == 0) break;
        if ((st == ST_FA_HDR || st == ST_FQ_HDR || st == ST_FQ_PLUS || st == ST_FQ_QUAL || st == ST_FQ_HSKIP) && c != '\n') {
            // skip to the end of this line in one go
            const void *nl = memchr(bytes + i, '\n', len - i);
            const size_t j = nl ? (size_t)(static_cast<const uint8_t *>(nl) - bytes) : len;
            if (memchr(bytes + i, 0, j - i)) break;  // a NUL inside the skipped text ends the input
            if (j >= len) break;
            i = j - 1;  // the newline itself goes through the state machine
            continue;
        }
        switch (st) {
        case ST_INIT:
            if (c == '>') st = ST_FA_HDR;
            else if (c == '@') st = ST_FQ_HDR;
            break;
        case ST_FA_HDR:
            if (c == '\n') { st = ST_FA_SEQ; put_break(); }
            break;
        case ST_FQ_HDR:
            if (c == '\n') { st = ST_FQ_SEQ; put_break(); }
            break;
        case ST_FA_SEQ:
        case ST_FQ_SEQ: {
            // fast path: a run of base bytes is copied in one go (vectorisable scan, no table look-up)
            if (is_base_byte(c)) {
                const size_t j = i + base_run_length(bytes + i, len - i);
                memcpy(out + o, bytes + i, j - i);
                o += j - i;
                last_break = false;
                i = j - 1;
                break;
            }
            const uint8_t cl = g_cls.t[c];
            if (cl == CL_BASE) {
                out[o++] = c;
                last_break = false;
            } else if (st == ST_FA_SEQ && c == '>') {
                put_break();
                st = ST_FA_HDR;
            } else if (cl == CL_SKIP) {
                if (st == ST_FQ_SEQ && c == '\n' && i + 1 < len) {
                    const uint8_t c2 = bytes[++i];  // the byte after a sequence newline is consumed
                    if (c2 == 0) return finish();
                    if (c2 == '+') st = ST_FQ_PLUS;
                }
            } else {
                put_break();
            }
            break;
        }
        case ST_FQ_PLUS:
            if (c == '\n') st = ST_FQ_QUAL;
            break;
        case ST_FQ_QUAL:
            if (c == '\n') st = ST_FQ_H;
            break;
        case ST_FQ_H:
            if (c == '@') { st = ST_FQ_HDR; put_break(); }
            else st = ST_FQ_HSKIP;
            break;
        case ST_FQ_HSKIP:
            if (c == '\n') st = ST_FQ_H;
            break;
        }
    }
    return finish();
}

int64_t frame_sequence_host(const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap)
{
    return frame_sequence_counting(bytes, len, out, out_cap, 0, nullptr);
}

extern "C" int64_t psk_frame_sequence(const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap)
{
    if ((!bytes && len) || !out) return PSK_EINVAL;
    return frame_sequence_host(bytes, len, out, out_cap);
}

// frames `bytes` into `stage` (host, thread-safe) and pads it for the extract kernel
int frame_into(uint8_t *stage, size_t stage_cap, const uint8_t *bytes, size_t len, uint64_t *clean_len, uint64_t *padded_len, int k,
               uint64_t *n_windows)
{
    int64_t n = frame_sequence_counting(bytes, len, stage, stage_cap, k, n_windows);
    if (n < 0) return (int)n;
    const uint64_t padded = ((uint64_t)n + EX_SEG - 1) / EX_SEG * EX_SEG + EX_SEG;
    memset(stage + n, '\n', padded - n);
    *clean_len = (uint64_t)n;
    *padded_len = padded;
    return PSK_OK;
}
