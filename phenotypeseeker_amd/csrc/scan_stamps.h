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
//
// Since r31 a single-kernel scan of at most STAMP_SUMMARY_MAX_GRID workgroups writes no clock word per segment, and the
// host does not wait for its count words: the scan's LAST publisher (stamp_ticket_*, below) writes a summary into the
// padding behind the start clock, on the start clock's own 64-byte line --
//   word STAMP_SUM_END   launch number (low 16 bits) << 48 | the wall clock when the last segment was published
//   word STAMP_SUM_LO    launch number (low 32 bits) << 32 | low 32 bits of the scan's survivors (n_pass)
//   word STAMP_SUM_HI    launch number (low 32 bits) << 32 | STAMP_SUM_OVERFLOW | bits 32 ... 39 of n_pass
// -- and psk_scan_end polls that one line (stamp_summary_ready).  The count words are still written, one per segment by the
// segment's publisher, and read when a result call asks for them.  A larger launch writes the segments' clock words and
// no summary, and is waited for word by word as before.  Every function the header had before r31 is kept, also those
// the driver does not call (stamp_counts_ready, stamp_clocks_ready): tests/scan_stamps_check.cpp compiles against them.
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

// ---- the summary line ------------------------------------------------------------------------------------------------
// indices into a set's STAMP_SET_WORDS block: the padding words behind the start clock (word 2 * STAMP_NSEG, line-aligned)
constexpr int STAMP_SUM_START = 2 * STAMP_NSEG;          // the start clock, as before
constexpr int STAMP_SUM_END = STAMP_SUM_START + 1;
constexpr int STAMP_SUM_LO = STAMP_SUM_START + 2;
constexpr int STAMP_SUM_HI = STAMP_SUM_START + 3;
static_assert(STAMP_SUM_HI < STAMP_SET_WORDS && STAMP_SUM_START % 8 == 0, "the summary shares the start clock's 64-byte line");
constexpr uint64_t STAMP_NPASS_MAX = (1ull << 40) - 1;   // STAMP_NSEG segments of fewer than 2^32 survivors each
constexpr uint32_t STAMP_SUM_OVERFLOW = 1u << 31;        // flag of the high word: some segment's count exceeded its capacity

STAMP_SHARED uint64_t stamp_sum_lo_word(uint32_t seq, uint64_t n_pass) { return stamp_count_word(seq, (uint32_t)n_pass); }
STAMP_SHARED uint64_t stamp_sum_hi_word(uint32_t seq, uint64_t n_pass, bool overflow)
{
    return stamp_count_word(seq, (uint32_t)((n_pass & STAMP_NPASS_MAX) >> 32) | (overflow ? STAMP_SUM_OVERFLOW : 0u));
}
STAMP_SHARED uint64_t stamp_sum_n_pass(uint64_t lo, uint64_t hi) { return ((uint64_t)(stamp_word_count(hi) & 0xffu) << 32) | stamp_word_count(lo); }
STAMP_SHARED bool stamp_sum_overflow(uint64_t hi) { return (stamp_word_count(hi) & STAMP_SUM_OVERFLOW) != 0; }

// The ticket line: one u64 on the device that every publisher of a scan adds to ONCE with its segment's count c, in one
// atomic that returns the sum so far -- bits 0 ... 39 the survivors, bits 40 ... 51 the publishers that have added, bits
// 52 ... 63 how many of them saw c > seg_cap (a count, so that it never falls back to zero: "sticky").  A scan has
// min(workgroups, STAMP_NSEG) publishers: one per segment that some workgroup maps to.  The publisher whose atomic
// returns publishers - 1 tickets is the last; the value returned plus its own addend is the whole scan's.
// Only launches of at most STAMP_SUMMARY_MAX_GRID workgroups take tickets and write a summary (the flagship launch has 28);
// a larger launch stamps a clock beside every segment's count, as all did until r31, and the host waits for those.  The
// ticket is a dependent atomic round trip in the kernel's tail, 0.4-0.5 us, and 256 publishers on the one address cost
// another 0.9 us: the kernels of 256 and more workgroups ran 1.1-1.7 us longer with it (NOTEBOOK r31).
constexpr uint32_t STAMP_SUMMARY_MAX_GRID = 64;
STAMP_SHARED bool stamp_summary_used(uint32_t workgroups) { return workgroups <= STAMP_SUMMARY_MAX_GRID; }
constexpr int STAMP_TICKET_SHIFT = 40, STAMP_TICKET_OVF_SHIFT = 52;
STAMP_SHARED uint32_t stamp_ticket_publishers(uint32_t workgroups) { return workgroups < (uint32_t)STAMP_NSEG ? workgroups : (uint32_t)STAMP_NSEG; }
STAMP_SHARED uint64_t stamp_ticket_addend(uint32_t c, uint32_t seg_cap)
{
    return (1ull << STAMP_TICKET_SHIFT) | (uint64_t)c | (c > seg_cap ? 1ull << STAMP_TICKET_OVF_SHIFT : 0ull);
}
STAMP_SHARED bool stamp_ticket_is_last(uint64_t before, uint32_t publishers) { return (uint32_t)((before >> STAMP_TICKET_SHIFT) & 0xfffu) == publishers - 1; }
STAMP_SHARED uint64_t stamp_ticket_total(uint64_t after) { return after & STAMP_NPASS_MAX; }
STAMP_SHARED bool stamp_ticket_overflow(uint64_t after) { return (after >> STAMP_TICKET_OVF_SHIFT) != 0; }

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

// the summary line of result set `set_words` carries launch `seq` in every one of its four words
inline bool stamp_summary_ready(const volatile uint64_t *set_words, uint32_t seq)
{
    return stamp_word_seq(stamp_load(set_words + STAMP_SUM_HI)) == seq && stamp_word_seq(stamp_load(set_words + STAMP_SUM_LO)) == seq &&
           stamp_clock_tag(stamp_load(set_words + STAMP_SUM_END)) == (seq & 0xffffu) && stamp_clock_tag(stamp_load(set_words + STAMP_SUM_START)) == (seq & 0xffffu);
}

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

// Ticks from the kernel's start clock to the end clock of its summary, by the same rule: an end before the start (the last
// publisher was not bound to run after workgroup 0 had read the clock) counts as one tick.
inline uint64_t stamp_summary_ticks(const volatile uint64_t *set_words)
{
    const uint64_t d = stamp_clock_diff(stamp_clock_value(stamp_load(set_words + STAMP_SUM_START)), stamp_clock_value(stamp_load(set_words + STAMP_SUM_END)));
    return d < (1ull << 47) && d > 1 ? d : 1;
}
