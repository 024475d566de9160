// The planning of a counting call (count_batch.hip, count_gz.hip) as plain arithmetic: nothing here touches the device or a
// file, so it can be read, compiled and checked on its own.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

// ---- one batch: host threads, buffer sets, pinned ring --------------------------------------------------------------------
struct psk_batch_plan {
    int n_threads = 1;      // worker threads that read / frame ahead
    int fill_helpers = 1;   // threads per large sample's copy into its pinned slot
    int G = 1;              // samples per launch chain (1: the one-sample chain)
    int n_sets = 3;         // buffer sets in rotation
    int R = 1;              // pinned ring slots
};

constexpr size_t PSK_GROUP_MAX_LEN = (size_t)64 << 20;   // samples from here on are read sets: one at a time, never grouped

// genomes at k <= 13 (dense counting) and k = 14..32 (bucketed sort) go through the counting kernels in groups: is this such a
// batch?  (the group-size knob, the free memory and the bytes per set are only asked for when it is)
inline bool psk_batch_may_group(int n, size_t max_len, bool dense, bool bucketed, bool consumer)
{
    return !consumer && (dense || bucketed) && n > 1 && max_len < PSK_GROUP_MAX_LEN;
}

// knob_G: what PSK_DC_GROUP gave; free_bytes, slab_cap, per_set: the device's free memory, what the slab of the buffer sets
// already holds (counts as free) and the bytes of ONE buffer set for max_len -- read only when the batch may group and knob_G > 1
inline psk_batch_plan psk_plan_batch(int n, size_t max_len, int n_threads, bool dense, bool bucketed, bool consumer, int knob_G,
                                     size_t free_bytes, size_t slab_cap, size_t per_set)
{
    psk_batch_plan p;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 16) n_threads = 16;
    p.fill_helpers = n_threads >= 2 * n ? n_threads / n : (n == 1 ? 8 : 1);
    // read sets (hundreds of MB a sample): the copies into pinned memory share the host's memory bandwidth, so six of
    // them at once all finish late and the first upload waits for them (r02: 6 x 0.63 GB, 87 ms before the first byte
    // moved, 137 ms in all).  One sample at a time with every thread on its copy finishes a sample every ~15 ms and the
    // uploads run beside the next copies.
    if (max_len >= PSK_GROUP_MAX_LEN && n > 1) {
        p.fill_helpers = n_threads > 8 ? 8 : n_threads;
        n_threads = 1;
    }
    if (n_threads > n) n_threads = n;
    // pinned ring: at most ~4 GiB of it (read-scale FASTQ samples are hundreds of MB each)
    while (n_threads > 1 && (size_t)(n_threads + 4) * max_len > (4ull << 30)) n_threads--;
    p.n_threads = n_threads;
    if (psk_batch_may_group(n, max_len, dense, bucketed, consumer)) p.G = knob_G;
    if (p.G > 1) {
        // The 3 G buffer sets of a grouped batch are one slab sized for the batch's longest sample: ~16 bytes per base on the
        // bucketed route -- 1.8 GB for 5-Mbp genomes, but 23 GB for samples just under the 64-MB grouping limit.
        // Smaller groups when the slab would pass a quarter of the device's free memory or 8 GiB; G = 1 is the one-sample
        // chain, which needs no slab at all.
        size_t cap = (free_bytes + slab_cap) / 4;
        if (cap > ((size_t)8 << 30)) cap = (size_t)8 << 30;
        while (p.G > 1 && (size_t)3 * p.G * per_set > cap) p.G /= 2;
    }
    const bool grouped = p.G > 1;
    p.n_sets = grouped ? 3 * p.G : 3;
    // ring slots: two (groups) being uploaded / framed ahead, one whose chain is in flight, one released late (grouped: a slot
    // is released as soon as its upload is over) -- never more than there are samples
    const int want_ring = grouped ? p.G + n_threads + 4 : n_threads + 4;
    p.R = n < want_ring ? n : want_ring;
    return p;
}

// ---- the cut of a call into .gz runs ----------------------------------------------------------------------------------------
// A run: samples [lo, hi) of the call, cut where the text of its .gz samples (idx) would pass the budget; runs alternate
// between the two buffer sets.  isize[i]: ISIZE of sample i's last member (read only where is_gz[i]); a sample's text is
// taken as at least three times its image.
struct psk_gz_run_cut {
    int lo = 0, hi = 0, set = 0;
    std::vector<int> idx;
};

static inline std::vector<psk_gz_run_cut> psk_cut_gz_runs(int n, const char *is_gz, const size_t *lens, const size_t *isize, size_t budget)
{
    std::vector<psk_gz_run_cut> runs;
    for (int lo = 0; lo < n;) {
        psk_gz_run_cut r;
        r.lo = r.hi = lo;
        r.set = (int)runs.size() & 1;
        size_t est = 0;
        while (r.hi < n) {
            size_t e = 0;
            if (is_gz[r.hi]) {
                e = isize[r.hi];
                if (e < 3 * lens[r.hi]) e = 3 * lens[r.hi];
            }
            if (r.hi > lo && est + e > budget) break;
            est += e;
            if (is_gz[r.hi]) r.idx.push_back(r.hi);
            r.hi++;
        }
        lo = r.hi;
        runs.push_back(std::move(r));
    }
    return runs;
}
