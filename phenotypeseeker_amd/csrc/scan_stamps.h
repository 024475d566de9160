// How a scan tells the host that it is done, as plain arithmetic over words of pinned host memory: no HIP, no context, so it
// can be read, compiled and checked on its own (tests/scan_stamps_check.cpp).  The kernels write the words (scan_common.h:
// publish_segment, publish_segment_once, stamp_scan_start; the finalize kernels of the two-kernel scans), psk_scan_end
// polls them (chi2_driver.hip) and fetch_counts reads them (scan_results.hip).
//
// Per result set the block holds STAMP_NSEG count words and, behind them, STAMP_NSEG + 1 clock words:
//   count word of segment s   launch number (low 32 bits) << 32 | survivors of the segment
//   clock word of segment s   launch number (low 16 bits) << 48 | the device's wall clock (low 48 bits) when s was published
//   clock word STAMP_NSEG     the same when the kernel started
// Every word is one naturally aligned 8-byte store and carries its own tag, so a reader needs no ordering between words:
// a word whose tag is this scan's holds this scan's value, whatever else has or has not arrived.  Launch numbers start
// at 1 and the block starts zeroed, so no scan's tag matches a word that was never written.
// The clock words' tag is 16 bits and the two-kernel scans (weighted chi2, Welch) write no clock words, so a stamped scan
// whose result set last received clocks exactly 65,536 launches earlier would find that old scan's clocks "ready" and
// report ITS time.  Only the reported time: counts are matched on 32 bits, and the wait needs the counts first.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define STAMP_SHARED __host__ __device__ inline __attribute__((always_inline))
#else
#define STAMP_SHARED inline
#endif

constexpr int STAMP_NSEG = 256;                          // result segments of a scan (scan_common.h SC_NSEG)
constexpr int STAMP_CLOCKS = STAMP_NSEG + 1;             // one per segment and the kernel's start
constexpr int STAMP_START = STAMP_NSEG;                  // index of the start clock
constexpr int STAMP_SET_WORDS = 2 * STAMP_NSEG + 8;      // u64 of one result set: counts, clocks, padding to whole 64-byte lines
constexpr uint64_t STAMP_CLOCK_MASK = (1ull << 48) - 1;

STAMP_SHARED uint64_t stamp_count_word(uint32_t seq, uint32_t count) { return ((uint64_t)seq << 32) | count; }
STAMP_SHARED uint32_t stamp_word_seq(uint64_t w) { return (uint32_t)(w >> 32); }
STAMP_SHARED uint32_t stamp_word_count(uint64_t w) { return (uint32_t)w; }
STAMP_SHARED uint64_t stamp_clock_word(uint32_t seq, uint64_t clock) { return ((uint64_t)(seq & 0xffffu) << 48) | (clock & STAMP_CLOCK_MASK); }
STAMP_SHARED uint32_t stamp_clock_tag(uint64_t w) { return (uint32_t)(w >> 48); }
STAMP_SHARED uint64_t stamp_clock_value(uint64_t w) { return w & STAMP_CLOCK_MASK; }

// ---- the host's side -------------------------------------------------------------------------------------------------
// one word as the device left it: a single 8-byte load that the compiler may neither split nor keep in a register
inline uint64_t stamp_load(const volatile uint64_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// first segment at or after `from` whose count word does not carry seq yet; STAMP_NSEG: none, the counts are all here
inline int stamp_counts_missing(const volatile uint64_t *counts, uint32_t seq, int from = 0)
{
    int s = from;
    while (s < STAMP_NSEG && stamp_word_seq(stamp_load(counts + s)) == seq) s++;
    return s;
}
inline bool stamp_counts_ready(const volatile uint64_t *counts, uint32_t seq) { return stamp_counts_missing(counts, seq) == STAMP_NSEG; }

// the same over the STAMP_CLOCKS clock words and their 16-bit tag
inline int stamp_clocks_missing(const volatile uint64_t *clocks, uint32_t seq, int from = 0)
{
    int s = from;
    while (s < STAMP_CLOCKS && stamp_clock_tag(stamp_load(clocks + s)) == (seq & 0xffffu)) s++;
    return s;
}
inline bool stamp_clocks_ready(const volatile uint64_t *clocks, uint32_t seq) { return stamp_clocks_missing(clocks, seq) == STAMP_CLOCKS; }

// ticks from `start` to `end`, both 48-bit clock values: the counter may have wrapped once in between
inline uint64_t stamp_clock_diff(uint64_t start, uint64_t end) { return (end - start) & STAMP_CLOCK_MASK; }

// Ticks from the kernel's start to its last published segment.  A segment stamped before the start clock was read (the
// first workgroup is not bound to be the first to run) lies "2^48 less a little" after it: differences in the upper half
// of the range are such segments and count as none.  At least one tick: a scan is never reported as taking no time.
inline uint64_t stamp_scan_ticks(const volatile uint64_t *clocks)
{
    const uint64_t start = stamp_clock_value(stamp_load(clocks + STAMP_START));
    uint64_t most = 1;
    for (int s = 0; s < STAMP_NSEG; s++) {
        const uint64_t d = stamp_clock_diff(start, stamp_clock_value(stamp_load(clocks + s)));
        if (d < (1ull << 47) && d > most) most = d;
    }
    return most;
}
