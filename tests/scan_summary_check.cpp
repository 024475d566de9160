// Stand-alone check of the summary line of csrc/scan_stamps.h: the four words through which a single-kernel scan's last
// publisher tells the host that the scan has ended, its n_pass and its time, and the ticket arithmetic by which that
// publisher is found (run by tests/test_scan_summary_host.py, also under the thread and the address sanitizers; no GPU,
// no library).  The summary words round-trip at the ends of n_pass and either side of the 16-bit and 32-bit wraps of the
// launch number; "ready" refuses a line in which any one word is stale or was never written; of 1, 28, 256 or 257
// workgroups' publishers, in any order and with counts that add up past 2^32, exactly one draws the last ticket, and the
// sum it holds is the scan's, the overflow count included; and a reader that polls the line while another thread publishes
// launch after launch never takes a stale summary.  Integers and booleans throughout: no tolerance.
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

typedef unsigned long long ull;

// the device's store, as the host can make it: one relaxed 8-byte store
static void publish(volatile uint64_t *p, uint64_t w) { __atomic_store_n(p, w, __ATOMIC_RELAXED); }

static const uint32_t SEQS[] = {1u, 2u, 0xfffeu, 0xffffu, 0x10000u, 0x10001u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu, 0u, 1u + 0x10000u};
static const uint64_t NPASS[] = {0ull, 1ull, 1736ull, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 5, STAMP_NPASS_MAX};

static void fill_summary(std::vector<uint64_t> &blk, uint32_t seq, uint64_t n_pass, bool ovf, uint64_t start, uint64_t end)
{
    blk[STAMP_SUM_START] = stamp_clock_word(seq, start);
    blk[STAMP_SUM_END] = stamp_clock_word(seq, end);
    blk[STAMP_SUM_LO] = stamp_sum_lo_word(seq, n_pass);
    blk[STAMP_SUM_HI] = stamp_sum_hi_word(seq, n_pass, ovf);
}

static void check_words()
{
    CHECK(STAMP_SUM_START == STAMP_NSEG + STAMP_START, "the summary's start clock is the start clock: %d", STAMP_SUM_START);
    CHECK(STAMP_SUM_START * 8 % 64 == 0 && STAMP_SUM_HI / 8 == STAMP_SUM_START / 8 && STAMP_SUM_HI < STAMP_SET_WORDS, "one 64-byte line inside the set");
    for (uint32_t q : SEQS)
        for (uint64_t n : NPASS)
            for (int ovf = 0; ovf < 2; ovf++) {
                const uint64_t lo = stamp_sum_lo_word(q, n), hi = stamp_sum_hi_word(q, n, ovf != 0);
                CHECK(stamp_word_seq(lo) == q && stamp_word_seq(hi) == q, "seq %u n %llu: tags %u %u", q, (ull)n, stamp_word_seq(lo), stamp_word_seq(hi));
                CHECK(stamp_sum_n_pass(lo, hi) == n, "seq %u n %llu -> %llu", q, (ull)n, (ull)stamp_sum_n_pass(lo, hi));
                CHECK(stamp_sum_overflow(hi) == (ovf != 0), "seq %u n %llu overflow %d", q, (ull)n, ovf);
            }
}

// "ready" with each of the four words in turn left at another launch's tag, at the one a wrap ago, or at zero
static void check_ready()
{
    std::vector<uint64_t> blk(STAMP_SET_WORDS, 0);
    for (uint32_t q : SEQS) {
        std::fill(blk.begin(), blk.end(), 0ull);
        const volatile uint64_t *w = blk.data();
        if (q != 0) CHECK(!stamp_summary_ready(w, q), "seq %u: a zeroed line is ready", q);
        fill_summary(blk, q, 1736, false, 5000, 5400);
        CHECK(stamp_summary_ready(w, q), "seq %u: a full line is not ready", q);
        CHECK(stamp_summary_ticks(w) == 400, "seq %u: ticks %llu", q, (ull)stamp_summary_ticks(w));
        CHECK(!stamp_summary_ready(w, q + 1) && !stamp_summary_ready(w, q - 1), "seq %u: ready for a neighbour", q);
        CHECK(!stamp_summary_ready(w, q + 0x10000u) && !stamp_summary_ready(w, q - 0x10000u), "seq %u: ready for the launch a 16-bit wrap away", q);
        // the count words of the set play no part: whatever they hold, the line decides
        for (int s = 0; s < STAMP_NSEG; s++) blk[s] = stamp_count_word(q - 1, 7);
        CHECK(stamp_summary_ready(w, q), "seq %u: the count words were looked at", q);
        struct { int word; uint64_t stale; } cases[] = {
            {STAMP_SUM_START, stamp_clock_word(q - 1, 5000)}, {STAMP_SUM_START, stamp_clock_word(q + 1, 5000)}, {STAMP_SUM_START, (q & 0xffffu) ? 0ull : stamp_clock_word(1, 0)},
            {STAMP_SUM_END, stamp_clock_word(q - 1, 5400)}, {STAMP_SUM_END, stamp_clock_word(q + 1, 5400)}, {STAMP_SUM_END, (q & 0xffffu) ? 0ull : stamp_clock_word(1, 0)},
            {STAMP_SUM_LO, stamp_sum_lo_word(q - 1, 1736)}, {STAMP_SUM_LO, stamp_sum_lo_word(q - 0x10000u, 1736)}, {STAMP_SUM_LO, stamp_sum_lo_word(q ^ 0x80000000u, 1736)}, {STAMP_SUM_LO, q ? 0ull : stamp_sum_lo_word(1, 0)},
            {STAMP_SUM_HI, stamp_sum_hi_word(q - 1, 1736, false)}, {STAMP_SUM_HI, stamp_sum_hi_word(q - 0x10000u, 1736, true)}, {STAMP_SUM_HI, stamp_sum_hi_word(q ^ 0x80000000u, 1736, false)}, {STAMP_SUM_HI, q ? 0ull : stamp_sum_hi_word(1, 0, false)},
        };
        for (const auto &c : cases) {
            const uint64_t keep = blk[c.word];
            blk[c.word] = c.stale;
            CHECK(!stamp_summary_ready(w, q), "seq %u: ready with word %d at %#llx", q, c.word, (ull)c.stale);
            blk[c.word] = keep;
        }
        CHECK(stamp_summary_ready(w, q), "seq %u: the line was not restored", q);
    }
    // the time: across the clock's 48-bit wrap; an end before the start, or none after it, is one tick
    fill_summary(blk, 9, 0, false, STAMP_CLOCK_MASK - 99, 200);
    CHECK(stamp_summary_ticks(blk.data()) == 300, "ticks across the wrap %llu", (ull)stamp_summary_ticks(blk.data()));
    fill_summary(blk, 9, 0, false, 5000, 4990);
    CHECK(stamp_summary_ticks(blk.data()) == 1, "end before start: %llu", (ull)stamp_summary_ticks(blk.data()));
    fill_summary(blk, 9, 0, false, 5000, 5000);
    CHECK(stamp_summary_ticks(blk.data()) == 1, "no time at all: %llu", (ull)stamp_summary_ticks(blk.data()));
}

// One scan's publishers against a ticket line, as publish_summary (scan_common.h) runs them: every publisher adds its
// addend in one atomic; returns how many saw "last", and through `total` / `ovf` what the last one held.
static int run_tickets(std::atomic<uint64_t> &line, uint32_t workgroups, const std::vector<uint32_t> &counts, uint32_t seg_cap, const std::vector<int> &order,
                       uint64_t *total, bool *ovf, bool *sticky)
{
    const uint32_t pubs = stamp_ticket_publishers(workgroups);
    int lasts = 0;
    bool seen_ovf = false;
    *sticky = true;
    for (int i : order) {
        const uint64_t add = stamp_ticket_addend(counts[i], seg_cap);
        const uint64_t before = line.fetch_add(add, std::memory_order_relaxed), after = before + add;
        if (counts[i] > seg_cap) seen_ovf = true;
        if (stamp_ticket_overflow(after) != seen_ovf) *sticky = false;   // set by the first overflowed segment, and it stays
        if (stamp_ticket_is_last(before, pubs)) {
            lasts++;
            *total = stamp_ticket_total(after);
            *ovf = stamp_ticket_overflow(after);
            line.store(0, std::memory_order_relaxed);   // the re-arm
        }
    }
    return lasts;
}

static void check_tickets()
{
    CHECK(stamp_ticket_publishers(1) == 1 && stamp_ticket_publishers(28) == 28 && stamp_ticket_publishers(256) == 256 && stamp_ticket_publishers(257) == 256 &&
          stamp_ticket_publishers(0xffffffffu) == 256, "publishers are capped at the segments");
    std::mt19937 rng(31);
    std::atomic<uint64_t> line{0};
    const uint32_t grids[] = {1u, 28u, 256u, 257u};
    for (uint32_t grid : grids)
        for (int kind = 0; kind < 4; kind++)
            for (int rep = 0; rep < 8; rep++) {
                const uint32_t pubs = stamp_ticket_publishers(grid);
                const uint32_t seg_cap = kind == 2 ? 0xfffffff0u : 1000u;
                std::vector<uint32_t> counts(pubs);
                uint64_t want = 0;
                bool want_ovf = false;
                for (uint32_t i = 0; i < pubs; i++) {
                    // 0: small counts; 1: a few segments over their capacity; 2: counts that add up past 2^32 (and 2^39); 3: all empty
                    counts[i] = kind == 0 ? rng() % 1001u : kind == 1 ? (rng() % 5 == 0 ? 1001u + rng() % 100u : rng() % 1001u) : kind == 2 ? 0xfffffff0u - rng() % 16u : 0u;
                    want += counts[i];
                    want_ovf = want_ovf || counts[i] > seg_cap;
                }
                if (kind == 1 && !want_ovf) { want -= counts[0]; counts[0] = 1001u; want += counts[0]; want_ovf = true; }
                if (kind == 2 && pubs >= 2) CHECK(want > (1ull << 32), "the counts were meant to pass 2^32: %llu", (ull)want);
                std::vector<int> order(pubs);
                std::iota(order.begin(), order.end(), 0);
                std::shuffle(order.begin(), order.end(), rng);
                uint64_t total = ~0ull;
                bool ovf = false, sticky = false;
                const int lasts = run_tickets(line, grid, counts, seg_cap, order, &total, &ovf, &sticky);
                CHECK(lasts == 1, "grid %u kind %d: %d publishers saw the last ticket", grid, kind, lasts);
                CHECK(total == want, "grid %u kind %d: total %llu, want %llu", grid, kind, (ull)total, (ull)want);
                CHECK(ovf == want_ovf && sticky, "grid %u kind %d: overflow %d, want %d, sticky %d", grid, kind, (int)ovf, (int)want_ovf, (int)sticky);
                CHECK(line.load() == 0, "grid %u kind %d: the line was not re-armed", grid, kind);
                // what the last publisher writes goes through the summary words unchanged
                CHECK(stamp_sum_n_pass(stamp_sum_lo_word(7, total), stamp_sum_hi_word(7, total, ovf)) == want, "grid %u kind %d: n_pass through the words", grid, kind);
            }
    // every one of 256 full-capacity overflowed segments: the overflow count does not run into the sign or back to zero
    {
        std::vector<uint32_t> counts(256, 0xffffffffu);
        std::vector<int> order(256);
        std::iota(order.begin(), order.end(), 0);
        uint64_t total = 0;
        bool ovf = false, sticky = false;
        CHECK(run_tickets(line, 256, counts, 10, order, &total, &ovf, &sticky) == 1 && total == 256ull * 0xffffffffull && ovf && sticky, "256 overflowed segments: %llu", (ull)total);
        CHECK(total <= STAMP_NPASS_MAX, "the largest total fits the summary's 40 bits");
    }
    // the same with one thread per publisher
    for (uint32_t grid : grids) {
        const uint32_t pubs = stamp_ticket_publishers(grid);
        std::atomic<int> lasts{0};
        std::atomic<uint64_t> total{0};
        std::vector<std::thread> th;
        const uint32_t n_threads = pubs < 8 ? pubs : 8;
        for (uint32_t t = 0; t < n_threads; t++)
            th.emplace_back([&, t] {
                for (uint32_t i = t; i < pubs; i += n_threads) {
                    const uint64_t add = stamp_ticket_addend(0xfffffff0u + (i & 7u), 0xffffffffu);
                    const uint64_t before = line.fetch_add(add, std::memory_order_relaxed);
                    if (stamp_ticket_is_last(before, pubs)) { lasts++; total = stamp_ticket_total(before + add); line.store(0, std::memory_order_relaxed); }
                }
            });
        for (auto &t : th) t.join();
        uint64_t want = 0;
        for (uint32_t i = 0; i < pubs; i++) want += 0xfffffff0u + (i & 7u);
        CHECK(lasts == 1 && total == want && line.load() == 0, "grid %u, threads: %d lasts, total %llu, want %llu", grid, lasts.load(), (ull)total.load(), (ull)want);
    }
}

// One thread publishes the summary of launch after launch -- the start clock first, then the other three words in a
// shuffled order, one relaxed store each -- while this thread polls the way psk_scan_end does; whenever the poll says
// "ready", n_pass, the flag and the time must be the launch's own.
static void check_threads()
{
    std::vector<uint64_t> blk(STAMP_SET_WORDS, 0);
    volatile uint64_t *words = blk.data();
    const int LAUNCHES = 400;
    std::atomic<uint32_t> go{0}, seen{0};
    const uint32_t first = 0xffffu - 150;   // crosses the 16-bit wrap on the way
    auto n_of = [](uint32_t q) { return ((uint64_t)(q & 0xffu) << 32) | (q * 3u); };
    std::thread writer([&] {
        std::mt19937 rng(12345);
        int order[4] = {STAMP_SUM_START, STAMP_SUM_END, STAMP_SUM_LO, STAMP_SUM_HI};
        for (int i = 0; i < LAUNCHES; i++) {
            const uint32_t q = first + (uint32_t)i;
            while (go.load(std::memory_order_acquire) != q) std::this_thread::yield();
            std::shuffle(order, order + 4, rng);
            for (int w : order) {
                if (w == STAMP_SUM_START) publish(words + w, stamp_clock_word(q, (uint64_t)q * 1000));
                else if (w == STAMP_SUM_END) publish(words + w, stamp_clock_word(q, (uint64_t)q * 1000 + 77));
                else if (w == STAMP_SUM_LO) publish(words + w, stamp_sum_lo_word(q, n_of(q)));
                else publish(words + w, stamp_sum_hi_word(q, n_of(q), (q & 1u) != 0));
            }
            while (seen.load(std::memory_order_acquire) != q) std::this_thread::yield();
        }
    });
    for (int i = 0; i < LAUNCHES; i++) {
        const uint32_t q = first + (uint32_t)i;
        CHECK(i == 0 || !stamp_summary_ready(words, q), "launch %u ready before it was published", q);
        go.store(q, std::memory_order_release);
        long polls = 0;
        bool ready = false;
        for (;; polls++) {
            ready = stamp_summary_ready(words, q);
            if (ready || polls > 2000000000L) break;
            if ((polls & 63) == 63) std::this_thread::yield();
        }
        CHECK(ready, "launch %u never became ready", q);
        const uint64_t lo = stamp_load(words + STAMP_SUM_LO), hi = stamp_load(words + STAMP_SUM_HI);
        CHECK(stamp_sum_n_pass(lo, hi) == n_of(q) && stamp_sum_overflow(hi) == ((q & 1u) != 0), "launch %u: another launch's summary behind a ready poll", q);
        CHECK(stamp_summary_ticks(words) == 77, "launch %u: ticks %llu", q, (ull)stamp_summary_ticks(words));
        seen.store(q, std::memory_order_release);
    }
    writer.join();
}

int main()
{
    check_words();
    check_ready();
    check_tickets();
    check_threads();
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
