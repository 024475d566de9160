// Stand-alone check of csrc/scan_stamps.h, the words through which a scan's kernels tell the host their counts, that they
// are done and how long they took (run by tests/test_scan_stamps_host.py; no GPU, no library): the encodings round-trip,
// "ready" refuses a block in which any one word is another scan's or was never written -- either side of the wraps of
// the 16-bit and the 32-bit tag --, the clock difference crosses the 48-bit wrap, and a reader that polls while another
// thread publishes the words in a shuffled order sees "ready" only once every word is this scan's.  Integers and booleans
// throughout: no tolerance.
#include "../phenotypeseeker_amd/csrc/scan_stamps.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

static long n_checks = 0, n_fail = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        n_checks++;                                               \
        if (!(cond)) {                                            \
            if (n_fail++ < 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

// the device's store, as the host can make it: one relaxed 8-byte store
static void publish(volatile uint64_t *p, uint64_t w) { __atomic_store_n(p, w, __ATOMIC_RELAXED); }

static void fill(std::vector<uint64_t> &blk, uint32_t seq, uint64_t clock0)
{
    for (int s = 0; s < STAMP_NSEG; s++) blk[s] = stamp_count_word(seq, 1000u + (uint32_t)s);
    for (int s = 0; s < STAMP_CLOCKS; s++) blk[STAMP_NSEG + s] = stamp_clock_word(seq, clock0 + (s == STAMP_START ? 0 : 10 + s));
}

static void check_words()
{
    const uint32_t seqs[] = {1u, 2u, 0xfffeu, 0xffffu, 0x10000u, 0x10001u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu, 0u};
    const uint32_t counts[] = {0u, 1u, 1736u, 0x7fffffffu, 0xffffffffu};
    const uint64_t clocks[] = {0ull, 1ull, (1ull << 47), STAMP_CLOCK_MASK - 1, STAMP_CLOCK_MASK};
    for (uint32_t q : seqs) {
        for (uint32_t c : counts) {
            const uint64_t w = stamp_count_word(q, c);
            CHECK(stamp_word_seq(w) == q && stamp_word_count(w) == c, "seq %u count %u -> %#llx", q, c, (unsigned long long)w);
        }
        for (uint64_t t : clocks) {
            const uint64_t w = stamp_clock_word(q, t);
            CHECK(stamp_clock_tag(w) == (q & 0xffffu) && stamp_clock_value(w) == t, "seq %u clock %#llx -> %#llx", q, (unsigned long long)t, (unsigned long long)w);
        }
        // a clock wider than 48 bits keeps its low 48 and leaves the tag alone
        const uint64_t wide = stamp_clock_word(q, 0xabcd000000000123ull);
        CHECK(stamp_clock_tag(wide) == (q & 0xffffu) && stamp_clock_value(wide) == 0x123ull, "seq %u wide clock -> %#llx", q, (unsigned long long)wide);
    }
    CHECK(STAMP_SET_WORDS >= STAMP_NSEG + STAMP_CLOCKS && STAMP_SET_WORDS % 8 == 0, "%d words per set", STAMP_SET_WORDS);
}

// "ready" with every single word in turn left at the previous launch number, at the one a tag wrap ago, or at zero
static void check_ready()
{
    const uint32_t seqs[] = {1u, 2u, 0xffffu, 0x10000u, 0x10001u, 0x20000u, 0xffffffffu, 0u, 1u + 0x10000u};
    std::vector<uint64_t> blk(STAMP_SET_WORDS, 0);
    for (uint32_t q : seqs) {
        std::fill(blk.begin(), blk.end(), 0ull);
        const volatile uint64_t *counts = blk.data(), *clocks = blk.data() + STAMP_NSEG;
        if (q != 0) CHECK(!stamp_counts_ready(counts, q) && stamp_counts_missing(counts, q) == 0, "seq %u: a zeroed block is ready", q);
        if ((q & 0xffffu) != 0) CHECK(!stamp_clocks_ready(clocks, q), "seq %u: zeroed clocks are ready", q);
        fill(blk, q, 5000);
        CHECK(stamp_counts_ready(counts, q) && stamp_clocks_ready(clocks, q), "seq %u: a full block is not ready", q);
        CHECK(!stamp_counts_ready(counts, q + 1) && !stamp_counts_ready(counts, q - 1), "seq %u: ready for a neighbour", q);
        CHECK(!stamp_clocks_ready(clocks, q + 1) && !stamp_clocks_ready(clocks, q - 1), "seq %u: clocks ready for a neighbour", q);
        // the count words tell launches 65,536 apart from one another; the clock words' 16-bit tag cannot, and need not
        CHECK(!stamp_counts_ready(counts, q + 0x10000u), "seq %u: ready for the launch a 16-bit wrap later", q);
        CHECK(stamp_clocks_ready(clocks, q + 0x10000u), "seq %u: the clock tag is 16 bits", q);
        const uint64_t stale_counts[] = {stamp_count_word(q - 1, 7), stamp_count_word(q - 0x10000u, 7), stamp_count_word(q ^ 0x80000000u, 7), q ? 0ull : stamp_count_word(1, 0)};
        for (int s = 0; s < STAMP_NSEG; s++)
            for (uint64_t stale : stale_counts) {
                const uint64_t keep = blk[s];
                blk[s] = stale;
                CHECK(!stamp_counts_ready(counts, q) && stamp_counts_missing(counts, q) == s, "seq %u: ready with segment %d at %#llx", q, s, (unsigned long long)stale);
                CHECK(stamp_counts_missing(counts, q, s) == s && (s == 0 || stamp_counts_missing(counts, q, s - 1) == s), "seq %u: resumed poll at %d", q, s);
                blk[s] = keep;
            }
        const uint64_t stale_clocks[] = {stamp_clock_word(q - 1, 5000), stamp_clock_word(q + 1, 5000), (q & 0xffffu) ? 0ull : stamp_clock_word(1, 0)};
        for (int s = 0; s < STAMP_CLOCKS; s++)
            for (uint64_t stale : stale_clocks) {
                const uint64_t keep = blk[STAMP_NSEG + s];
                blk[STAMP_NSEG + s] = stale;
                CHECK(!stamp_clocks_ready(clocks, q) && stamp_clocks_missing(clocks, q) == s, "seq %u: clocks ready with word %d at %#llx", q, s, (unsigned long long)stale);
                blk[STAMP_NSEG + s] = keep;
            }
        CHECK(stamp_counts_ready(counts, q) && stamp_clocks_ready(clocks, q), "seq %u: the block was not restored", q);
    }
}

static void check_clock()
{
    CHECK(stamp_clock_diff(100, 350) == 250, "plain difference");
    CHECK(stamp_clock_diff(5, 5) == 0, "no difference");
    CHECK(stamp_clock_diff(STAMP_CLOCK_MASK - 9, 40) == 50, "across the 48-bit wrap: %llu", (unsigned long long)stamp_clock_diff(STAMP_CLOCK_MASK - 9, 40));
    CHECK(stamp_clock_diff(STAMP_CLOCK_MASK, 0) == 1, "one tick across the wrap");
    std::vector<uint64_t> blk(STAMP_SET_WORDS, 0);
    const volatile uint64_t *clocks = blk.data() + STAMP_NSEG;
    fill(blk, 9, 5000);   // segment s at start + 10 + s
    CHECK(stamp_scan_ticks(clocks) == 10 + STAMP_NSEG - 1, "ticks %llu", (unsigned long long)stamp_scan_ticks(clocks));
    fill(blk, 9, STAMP_CLOCK_MASK - 99);   // the counter wraps between the start and most segments
    CHECK(stamp_scan_ticks(clocks) == 10 + STAMP_NSEG - 1, "ticks across the wrap %llu", (unsigned long long)stamp_scan_ticks(clocks));
    blk[STAMP_NSEG + 17] = stamp_clock_word(9, STAMP_CLOCK_MASK - 99 + 70000);   // the last segment to arrive
    CHECK(stamp_scan_ticks(clocks) == 70000, "the largest segment clock decides: %llu", (unsigned long long)stamp_scan_ticks(clocks));
    // segments stamped before the start clock was read do not count; with nothing after the start, one tick
    fill(blk, 9, 5000);
    for (int s = 0; s < STAMP_NSEG; s++) blk[STAMP_NSEG + s] = stamp_clock_word(9, 4990);
    CHECK(stamp_scan_ticks(clocks) == 1, "all before the start: %llu", (unsigned long long)stamp_scan_ticks(clocks));
    blk[STAMP_NSEG + 3] = stamp_clock_word(9, 5400);
    CHECK(stamp_scan_ticks(clocks) == 400, "one after the start: %llu", (unsigned long long)stamp_scan_ticks(clocks));
}

// One thread publishes the 257 + 256 words of launch after launch in a shuffled order, one relaxed store each, while this
// thread polls the way psk_scan_end does; whenever the poll says "ready", every count must be the launch's own.
static void check_threads()
{
    std::vector<uint64_t> blk(STAMP_SET_WORDS, 0);
    volatile uint64_t *words = blk.data();
    const int LAUNCHES = 400;
    std::atomic<uint32_t> go{0}, seen{0};
    const uint32_t first = 0xffffu - 150;   // crosses the 16-bit wrap on the way
    std::thread writer([&] {
        std::mt19937 rng(12345);
        std::vector<int> order(STAMP_NSEG + STAMP_CLOCKS);
        for (int i = 0; i < LAUNCHES; i++) {
            const uint32_t q = first + (uint32_t)i;
            while (go.load(std::memory_order_acquire) != q) std::this_thread::yield();
            std::iota(order.begin(), order.end(), 0);
            std::shuffle(order.begin(), order.end(), rng);
            for (int w : order) {
                if (w < STAMP_NSEG) publish(words + w, stamp_count_word(q, q * 3u + (uint32_t)w));
                else publish(words + w, stamp_clock_word(q, (uint64_t)q * 1000 + (w - STAMP_NSEG == STAMP_START ? 0 : 1 + (w - STAMP_NSEG))));
            }
            while (seen.load(std::memory_order_acquire) != q) std::this_thread::yield();
        }
    });
    for (int i = 0; i < LAUNCHES; i++) {
        const uint32_t q = first + (uint32_t)i;
        CHECK(i == 0 || !stamp_counts_ready(words, q), "launch %u ready before it was published", q);
        go.store(q, std::memory_order_release);
        int nc = 0, nk = 0;
        long polls = 0;
        for (;; polls++) {
            nc = stamp_counts_missing(words, q, nc);
            if (nc == STAMP_NSEG) nk = stamp_clocks_missing(words + STAMP_NSEG, q, nk);
            if (nc == STAMP_NSEG && nk == STAMP_CLOCKS) break;
            if (polls > 2000000000L) break;
            if ((polls & 63) == 63) std::this_thread::yield();
        }
        CHECK(nc == STAMP_NSEG && nk == STAMP_CLOCKS, "launch %u never became ready", q);
        bool own = true;
        for (int s = 0; s < STAMP_NSEG; s++) {
            const uint64_t w = stamp_load(words + s);
            own = own && stamp_word_seq(w) == q && stamp_word_count(w) == q * 3u + (uint32_t)s;
        }
        CHECK(own, "launch %u: a count of another launch behind a ready poll", q);
        CHECK(stamp_scan_ticks(words + STAMP_NSEG) == STAMP_NSEG, "launch %u: ticks %llu", q, (unsigned long long)stamp_scan_ticks(words + STAMP_NSEG));
        seen.store(q, std::memory_order_release);
    }
    writer.join();
}

int main()
{
    check_words();
    check_ready();
    check_clock();
    check_threads();
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
