// a1: one counting call over samples in memory or on disk -- host threads read / frame ahead into a ring of pinned buffers while
// the calling thread drives the GPU half of the samples in order (count_chain.hip: chain_upload / chain_compute / chain_finalize).
//
// The window count is known from the framing (or bounded by it), so nothing has to come back from the GPU before a chain is
// launched; the only values the host needs -- the number of unique words, for the arena allocation -- are picked up
// late.  Two shapes of the loop (BatchRun):
//   one sample per chain (read sets, k >= 17, prediction's consumer, PSK_DC_GROUP=1): chain i is queued on buffer set i % 3,
//     then sample i - 1 is finalised (its event has long fired while chain i keeps the GPU busy); samples i + 1 and i + 2
//     are uploaded and framed ahead on their own streams;
//   groups of G = 8 genomes per chain (k <= 16, r03): 3 G buffer sets, a group's uploads and framing run ahead, one
//     launch chain counts the group (dense_group_enqueue / bucket_group_enqueue), the group before it is finalised meanwhile.
// uploads rotate over two copy streams (ctx->copy_streams, PSK_COPY_STREAMS = 1..4): with one, the next copy is only queued
// when the previous one has gone -- 256 genomes took 38-40 ms, with two 33-36 (r03; a stream per buffer set: set index mod streams)
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <mutex>

#include "count_plan.h"
#include "kmer_windows.h"   // EX_SEG: the padding of a clean stream
#include "psk_internal.h"

// Large samples (read sets: hundreds of MB) are moved into the pinned slot by several threads -- one thread copies
// at ~10 GB/s, which was the whole cost of a 0.63-GB FASTQ sample (60 ms of 61) -- and the same threads look for the
// NUL that ends the input.  src != nullptr: memcpy; else pread of `path`.  Returns 0, *nul_at = first NUL or len.
static int parallel_fill(uint8_t *dst, const uint8_t *src, const char *path, size_t len, int helpers, size_t *nul_at)
{
    if (helpers < 1) helpers = 1;
    if (helpers > 16) helpers = 16;
    int fd = -1;
    if (!src) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return -1;
    }
    std::vector<size_t> nul((size_t)helpers, len);
    std::vector<int> bad((size_t)helpers, 0);
    const size_t slice = ((len + helpers - 1) / helpers + 4095) & ~size_t(4095);
    auto work = [&](int h) {
        const size_t lo = (size_t)h * slice, hi = lo + slice < len ? lo + slice : len;
        if (lo >= hi) return;
        if (src) memcpy(dst + lo, src + lo, hi - lo);
        else {
            size_t got = lo;
            while (got < hi) {
                const ssize_t r = pread(fd, dst + got, hi - got, (off_t)got);
                if (r <= 0) { bad[h] = 1; return; }
                got += (size_t)r;
            }
        }
        const void *z = memchr(dst + lo, 0, hi - lo);
        if (z) nul[h] = (size_t)(static_cast<const uint8_t *>(z) - dst);
    };
    std::vector<std::thread> ts;
    for (int h = 1; h < helpers; h++) ts.emplace_back(work, h);
    work(0);
    for (auto &t : ts) t.join();
    if (fd >= 0) close(fd);
    size_t first = len;
    for (int h = 0; h < helpers; h++) { if (bad[h]) return -1; if (nul[h] < first) first = nul[h]; }
    *nul_at = first;
    return 0;
}

namespace {

// One run of the batch counter.  The worker threads fill ring slot i % R with sample i and publish it in state[i]; the calling
// thread takes the samples in order through stage A (upload + GPU framing) and stage B (the counting chain), finalises them one
// sample (or group) late and gives the slots back with release_upto.  `rc` is the call's result so far: once it is not PSK_OK
// no further stage is started and the next release_upto tells the workers to stop.
struct BatchRun {
    psk_ctx *ctx;
    const CountRequest &q;
    const int n, k;
    psk_batch_plan plan;
    int NL = 3, R = 1;                     // buffer sets in rotation, ring slots
    bool bucket_run = false, gpu_framing = true;
    size_t max_len = 0, slot_need = 0;

    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> state;                // 0 pending, 1 ready, -1 reading / framing failed, -2 a gzip image, -3 no pinned memory
    std::vector<int> fmt;                  // 0 the ring slot holds a clean stream (host framing); 1 / 2 raw FASTA / FASTQ bytes
    std::vector<char> pre_up;              // (grouped batches) a windowless sample's clean stream is already in its set's buffer
    std::vector<uint64_t> clen, plen, wins, roff, rlen;
    int consumed = 0;                      // samples whose ring slot may be overwritten
    bool abort = false;                    // the workers stop at their next wait
    int rc = PSK_OK;
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    int next_a = 0, released = 0;          // (grouped) the next sample of stage A; ring slots given back so far
    // PSK_TRACE: where the calling thread waits (stderr, one line per call)
    double t_worker = 0, t_frame = 0, t_final = 0, t_setup = 0;
    std::atomic<long long> t_fill_us{0};
    Stopwatch t_call;

    BatchRun(psk_ctx *c, const CountRequest &req)
        : ctx(c), q(req), n(req.n), k(req.consumer ? req.k_window : c->k), state(n, 0), fmt(n, 0), pre_up(n, 0), clen(n, 0), plen(n, 0),
          wins(n, 0), roff(n, 0), rlen(n, 0) {}
    // every way out: the workers are told to stop and joined, and nothing of a grouped batch stays switched on in the context
    ~BatchRun()
    {
        stop_workers();
        ctx->dense_defer = false;
        for (CountLane &L : ctx->lane) { L.group_pending = false; L.dc_defer_compact = false; }
    }

    bool on_device(int i) const { return q.gzs && q.gzs[i].dev != nullptr; }
    const uint8_t *bytes_of(int i) const { return q.bytes ? q.bytes[i] : nullptr; }
    const char *path_of(int i) const { return (q.bytes && q.bytes[i]) || !q.paths ? nullptr : q.paths[i]; }
    int sample_of(int i) const { return q.first_sample_idx + i; }
    CountLane &lane_of(int i) { return ctx->lane[i % NL]; }
    bool grouped() const { return plan.G > 1; }

    int make_plan()
    {
        // every sample takes the pipelined path (chain_upload / chain_compute); with a slab filter the host's window count is
        // an upper bound and the kernels read the number of kept words from device memory
        for (int i = 0; i < n; i++) {
            if (!on_device(i) && !bytes_of(i) && !path_of(i) && q.lens[i]) return psk_fail(ctx, PSK_EINVAL, "null input %d", i);
            if (q.lens[i] > max_len) max_len = q.lens[i];
        }
        bucket_run = !ctx->dense_mode && ctx->k >= 14 && ctx->k <= 32 && !env_flag("PSK_NO_BUCKET_SORT");
        int knob_G = 1;
        size_t free_b = 0, total_b = 0, per_set = 0;
        if (psk_batch_may_group(n, max_len, ctx->dense_mode, bucket_run, q.consumer != nullptr)) {
            PSK_TRY(dense_group_size(ctx, &knob_G));
            if (knob_G > 1) {
                // (what the context already holds counts as free; frames on the GPU unless PSK_HOST_FRAMING: the larger of the two
                // layouts is budgeted)
                if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
                per_set = lane_set_bytes(ctx, max_len, true);
            }
        }
        plan = psk_plan_batch(n, max_len, q.n_threads, ctx->dense_mode, bucket_run, q.consumer != nullptr, knob_G, free_b, ctx->lane_slab.cap, per_set);
        NL = plan.n_sets;
        R = plan.R;
        if ((int)ctx->ring.size() < R) { ctx->ring.resize(R, nullptr); ctx->ring_cap.resize(R, 0); }
        // A slot that is missing or too small is pinned by the worker that first fills it (sample i < R is the first user of slot
        // i, and nobody else touches the slot before that sample is ready) -- r04: all R slots up front, ~2 ms of page pinning each,
        // were 16-40 ms in front of the first upload of a process's first calls (20 slots for 5-Mbp genomes); now the first upload
        // waits for one slot and the others are pinned beside it, by the threads that would otherwise wait for their turn
        size_t max_host_len = 0;   // (the text of a .gz sample inflated on the device needs no pinned slot)
        bool any_host = false;
        for (int i = 0; i < n; i++)
            if (!on_device(i)) {
                any_host = true;
                if (q.lens[i] > max_host_len) max_host_len = q.lens[i];
            }
        slot_need = any_host ? max_host_len + 2 * EX_SEG : 0;
        // FASTA and four-line FASTQ are framed on the GPU (frame_gpu.hip): the worker threads then only move file bytes
        // into pinned memory.  PSK_HOST_FRAMING=1 keeps the host state machine for everything (A/B runs, tests).
        gpu_framing = !env_flag("PSK_HOST_FRAMING");
        t_call = Stopwatch();   // (PSK_TRACE counts from here)
        return PSK_OK;
    }

    void start_workers()
    {
        for (int t = 0; t < plan.n_threads; t++) pool.emplace_back([this] { worker(); });
    }

    void stop_workers()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            abort = true;
        }
        cv.notify_all();
        for (auto &t : pool) t.join();
        pool.clear();
    }

    void worker()
    {
        std::vector<uint8_t> file_buf;  // file image of the sample in hand (paths form, host framing)
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) return;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return abort || consumed > i - R; });  // slot i % R is free again
                if (abort) return;
            }
            uint64_t c = 0, p = 0, w = 0, ro = 0, rl = 0;
            int frc = 0, f = 0;
            if (slot_need && i < R && (!ctx->ring[i] || ctx->ring_cap[i] < slot_need)) {
                if (hipSetDevice(ctx->device) != hipSuccess || ensure_pinned(ctx, &ctx->ring[i], &ctx->ring_cap[i], slot_need) != PSK_OK) frc = -3;
            }
            uint8_t *slot = static_cast<uint8_t *>(ctx->ring[i % R]);
            if (frc) {
                // (no pinned memory: reported by stage A)
            } else if (on_device(i)) {
                f = q.gzs[i].fmt;
                ro = q.gzs[i].roff;
                rl = q.gzs[i].rlen;
            } else if (gpu_framing) {
                // file bytes straight into the pinned slot (by several threads when the sample is large and threads
                // are idle); the probe finds where the records start and end
                size_t nul_at = q.lens[i];
                const Stopwatch tf;
                frc = parallel_fill(slot, bytes_of(i), path_of(i), q.lens[i], q.lens[i] >= (32u << 20) ? plan.fill_helpers : 1, &nul_at);
                t_fill_us += (long long)(tf.s() * 1e6);
                if (frc == 0 && path_of(i) && q.lens[i] >= 2 && slot[0] == 0x1f && slot[1] == 0x8b) frc = -2;   // gzip (PSK_NO_GPU_GZ): the caller inflates
                if (frc == 0) {
                    size_t st = 0, en = 0;
                    f = frame_probe_known_end(slot, nul_at, &st, &en);   // parallel_fill has found the NUL, if any
                    ro = st;
                    rl = en - st;
                }
            } else {
                const uint8_t *src = bytes_of(i);
                if (path_of(i)) {
                    file_buf.resize(q.lens[i] ? q.lens[i] : 1);
                    frc = read_exact(path_of(i), 0, q.lens[i], file_buf.data());
                    src = file_buf.data();
                    if (frc == 0 && q.lens[i] >= 2 && src[0] == 0x1f && src[1] == 0x8b) frc = -2;
                }
                if (frc == 0) frc = frame_into(slot, ctx->ring_cap[i % R], src, q.lens[i], &c, &p, k, &w);
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                clen[i] = c; plen[i] = p; wins[i] = w; fmt[i] = f; roff[i] = ro; rlen[i] = rl;
                state[i] = frc == -2 ? -2 : frc == -3 ? -3 : frc ? -1 : 1;
            }
            cv.notify_all();
        }
    }

    // ring slots of the samples before `upto` may be overwritten; a call that has failed stops its workers here
    void release_upto(int upto)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            consumed = upto;
            if (rc != PSK_OK) abort = true;
        }
        cv.notify_all();
    }

    void report(int i)
    {
        if (q.n_unique) q.n_unique[i] = ctx->lists[sample_of(i)].n_unique;
        if (q.n_total) q.n_total[i] = ctx->lists[sample_of(i)].n_total;
    }

    int collect_sketch(int i)
    {
        CountLane &L = lane_of(i);
        if (wins[i] == 0) {
            // no window of the counting k, so nothing was counted -- but the sketch's k may be shorter: take the
            // clean stream (host framing: from the ring slot, still held) through the synchronous route
            q.n_hashes_out[i] = 0;
            L.sk_state = 0;
            if (clen[i] == 0) return PSK_OK;
            if (fmt[i] == 0 && !pre_up[i]) {
                PSK_TRY(dev_reserve(ctx, L.raw, plen[i]));
                PSK_HIP(ctx, hipMemcpyAsync(L.raw.p, ctx->ring[i % R], plen[i], hipMemcpyHostToDevice, ctx->stream));
            }
            L.sk_state = 2;
        }
        return sketch_collect(ctx, L, L.raw.as<uint8_t>(), clen[i], q.sketch_k, q.sketch_size, q.sketch_seed,
                              q.hashes_out + (size_t)i * q.sketch_size, q.n_hashes_out + i);
    }

    // stage A of sample i (waits for its worker): upload + GPU framing on the copy stream
    int stage_a(int i)
    {
        {
            const Stopwatch t0;
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[i] != 0; });
            t_worker += t0.s();
            if (state[i] == -2)
                return psk_fail(ctx, PSK_EGZIP, "sample %d (%s) is gzip-compressed: inflate it and use the in-memory call",
                                sample_of(i), path_of(i) ? path_of(i) : "");
            if (state[i] == -3) return psk_fail(ctx, PSK_ENOMEM, "no pinned memory for sample %d (hipHostMalloc of %zu bytes failed)", sample_of(i), slot_need);
            if (state[i] < 0)
                return psk_fail(ctx, PSK_ERANGE, path_of(i) ? "reading or framing sample %d (%s) failed" : "framing of sample %d failed",
                                sample_of(i), path_of(i) ? path_of(i) : "");
        }
        if (on_device(i) && fmt[i]) return chain_upload(ctx, lane_of(i), q.gzs[i].dev + roff[i], rlen[i], fmt[i], true);
        const uint8_t *slot = static_cast<const uint8_t *>(ctx->ring[i % R]);
        if (fmt[i]) return chain_upload(ctx, lane_of(i), slot + roff[i], rlen[i], fmt[i]);
        if (wins[i] >= (1ull << 32)) return psk_fail(ctx, PSK_ERANGE, "sample with more than 2^32 windows");
        return chain_upload(ctx, lane_of(i), slot, wins[i] ? plen[i] : 0, 0);
    }

    // the counting chain, or the consumer in its place (its callers count from 0; a call cut into runs goes on counting)
    int consume(CountLane &L, int i, uint64_t clean_len, uint64_t n_windows, bool exact)
    {
        if (q.consumer) return (clean_len && n_windows) ? (*q.consumer)(L, sample_of(i), clean_len) : PSK_OK;
        return chain_compute(ctx, L, sample_of(i), clean_len, n_windows, exact);
    }

    // stage B: the counting chain, once the length of the clean stream is known on the host
    int stage_b(int i)
    {
        CountLane &L = lane_of(i);
        if (!(fmt[i] && rlen[i])) return consume(L, i, clen[i], wins[i], true);
        const Stopwatch t0;
        PSK_HIP(ctx, hipEventSynchronize(L.raw_ready));   // the GPU is busy with the chain of sample i - 1 meanwhile
        t_frame += t0.s();
        const uint64_t *res = lane_frame_result(L);
        if (fmt[i] == 2 && res[1] && env_flag("PSK_HOST_WRAPPED_FASTQ")) {
            // (r05's route, kept as the A/B knob: the host state machine frames a FASTQ sample that is not four-line FASTQ)
            PSK_TRY(ensure_pinned(ctx, &ctx->pinned, &ctx->pinned_cap, rlen[i] + 2 * EX_SEG));
            uint64_t c = 0, p = 0, w = 0;
            std::vector<uint8_t> text;   // (a .gz sample inflated on the device: its text comes back for the host's state machine)
            const uint8_t *records = on_device(i) ? nullptr : static_cast<const uint8_t *>(ctx->ring[i % R]) + roff[i];
            if (!records) {
                text.resize(rlen[i]);
                PSK_HIP(ctx, hipMemcpy(text.data(), q.gzs[i].dev + roff[i], rlen[i], hipMemcpyDeviceToHost));
                records = text.data();
            }
            const int frc = frame_into(static_cast<uint8_t *>(ctx->pinned), ctx->pinned_cap, records, rlen[i], &c, &p, k, &w);
            if (frc) return psk_fail(ctx, frc, "framing of sample %d failed", sample_of(i));
            clen[i] = c; plen[i] = p; wins[i] = w; fmt[i] = 0;
            PSK_TRY(chain_upload(ctx, L, static_cast<const uint8_t *>(ctx->pinned), w ? p : 0, 0));
            PSK_HIP(ctx, hipEventSynchronize(L.raw_ready));   // ctx->pinned is reused by the next such sample
            return consume(L, i, c, w, true);
        }
        if (fmt[i] == 2 && res[1]) {
            // not four-line FASTQ (records over several lines, blank lines between them): framed again, on the device, by the
            // scan of line kinds (frame_gpu.hip, format 3; r06 -- until then the host's state machine took such a sample); the
            // raw bytes are still in the lane's input buffer
            if (env_flag("PSK_TRACE"))
                fprintf(stderr, "[psk] sample %d: FASTQ, but not four lines a record: framed on the device by the scan of line kinds\n", sample_of(i));
            PSK_TRY(frame_gpu_enqueue(ctx, ctx->frame_stream, 3, L.rawin.as<uint8_t>(), rlen[i], L.raw.as<uint8_t>(), L.fr_scratch.p, lane_frame_result(L)));
            PSK_HIP(ctx, hipEventRecord(L.raw_ready, ctx->frame_stream));
            PSK_HIP(ctx, hipEventSynchronize(L.raw_ready));
            res = lane_frame_result(L);
        }
        clen[i] = res[0];
        wins[i] = res[0];   // an upper bound of the window count: sizes the buffers, the GPU counts the windows
        return consume(L, i, clen[i], wins[i], false);
    }

    // (grouped) the copy stream is kept ahead: stage A of the samples before `upto`
    void pump_a(int upto)
    {
        while (rc == PSK_OK && next_a < n && next_a < upto) rc = stage_a(next_a++);
    }

    // (grouped) the group [lo, hi) whose chain was queued one group ago: sizes read back, multi-count blocks allocated, one
    // compaction launch, sketches collected -- which frees its buffer sets for the group after next
    int finalize_group(int lo, int hi)
    {
        CountLane *gl[8];
        int gs[8], cnt = 0;
        const Stopwatch t0;
        for (int i = lo; i < hi; i++) {
            CountLane &L = lane_of(i);
            PSK_TRY(chain_finalize(ctx, L));
            if (L.dc_defer_compact) { gl[cnt] = &L; gs[cnt] = sample_of(i); cnt++; }   // sized and allocated; packed below
        }
        if (cnt) PSK_TRY(ctx->dense_mode ? dense_group_compact(ctx, gl, gs, cnt) : bucket_group_compact(ctx, gl, gs, cnt));
        t_final += t0.s();
        for (int i = lo; i < hi; i++) {
            report(i);
            if (q.sketch_k) PSK_TRY(collect_sketch(i));
        }
        if (hi > released) { released = hi; release_upto(hi); }
        return PSK_OK;
    }

    // Groups of G samples: a group's uploads and framing run two groups ahead on the copy / framing streams; its samples'
    // host halves (the framed length, the arena blocks) are done one by one, then ONE launch chain counts the group
    // (dense_group_enqueue); the group before it is finalised meanwhile.
    void run_grouped()
    {
        const int G = plan.G;
        ctx->dense_defer = true;
        pump_a(G);
        int prev_lo = -1, prev_hi = -1;
        for (int lo = 0, hi = 0; lo < n && rc == PSK_OK; lo = hi) {
            // (k = 14..16: the first sample of a run goes through the radix route alone and is finalised at once -- its list
            // gives the splitters of the bucketed sort that every later sample, grouped, takes)
            const bool alone = bucket_run && !ctx->bs_ready;
            hi = alone ? lo + 1 : (lo + G < n ? lo + G : n);
            CountLane *gl[8];
            int gs[8], cnt = 0;
            uint64_t gc[8], gn[8];
            for (int i = lo; i < hi && rc == PSK_OK; i++) {
                rc = stage_b(i);   // a genome's chain stays pending; anything else (an empty sample, a read set) is queued here
                CountLane &L = lane_of(i);
                // the pinned slot goes back as soon as the upload is over (framed on the GPU: stage B has waited for the
                // framing; framed on the host: wait for the copy here -- it ran G samples ahead), so the ring needs G + a few
                // slots, not three groups' worth (a cold context pays ~2 ms per pinned slot).  A sample too short for a
                // window of the counting k whose sketch will still want its clean stream: uploaded now.
                if (rc == PSK_OK && !fmt[i] && wins[i] > 0 && hipEventSynchronize(L.raw_ready) != hipSuccess)
                    rc = psk_fail(ctx, PSK_EHIP, "event wait failed");
                if (rc == PSK_OK && q.sketch_k && wins[i] == 0 && fmt[i] == 0 && clen[i]) {
                    rc = dev_reserve(ctx, L.raw, plen[i]);
                    if (rc == PSK_OK && (hipMemcpyAsync(L.raw.p, ctx->ring[i % R], plen[i], hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                                         hipStreamSynchronize(ctx->stream) != hipSuccess))
                        rc = psk_fail(ctx, PSK_EHIP, "upload of a short sample failed");
                    pre_up[i] = 1;
                }
                if (rc == PSK_OK) { released = i + 1; release_upto(released); }
                // the copy stream is kept G samples ahead (their buffer sets are those of the group before last: finalised)
                pump_a(i + 1 + G);
                if (rc == PSK_OK && L.group_pending) {
                    L.group_pending = false;
                    gl[cnt] = &L; gs[cnt] = sample_of(i); gc[cnt] = L.clean_len; gn[cnt] = L.n;
                    cnt++;
                }
            }
            if (rc == PSK_OK && cnt) rc = ctx->dense_mode ? dense_group_enqueue(ctx, gl, gs, gc, gn, cnt) : bucket_group_enqueue(ctx, gl, gs, gc, gn, cnt);
            for (int i = lo; i < hi && rc == PSK_OK; i++)
                if (q.sketch_k && wins[i] > 0)
                    rc = sketch_enqueue(ctx, lane_of(i), lane_of(i).raw.as<uint8_t>(), clen[i], q.sketch_k, q.sketch_size, q.sketch_seed);
            if (rc == PSK_OK && prev_lo >= 0) rc = finalize_group(prev_lo, prev_hi);
            prev_lo = lo; prev_hi = hi;
            if (rc == PSK_OK && alone) { rc = finalize_group(lo, hi); prev_lo = -1; }
        }
        if (rc == PSK_OK && prev_lo >= 0) rc = finalize_group(prev_lo, prev_hi);
    }

    // Samples i + 1 and i + 2 are uploaded and framed on the copy stream while chain i runs: the host's wait for the
    // framed length of sample i (stage B) then finds it long done (with one sample ahead the wait sat on the critical
    // path: 200 us per 5-Mbp sample instead of 145).
    void run_one_by_one()
    {
        rc = stage_a(0);
        if (rc == PSK_OK && n > 1) rc = stage_a(1);
        for (int i = 0; i < n && rc == PSK_OK; i++) {
            rc = stage_b(i);
            if (rc == PSK_OK && i > 0) {
                const Stopwatch t0;
                if (q.consumer) {   // no list to finalise: the upload of sample i - 1 has to be over before its ring slot is reused
                    if (hipEventSynchronize(lane_of(i - 1).raw_ready) != hipSuccess) rc = psk_fail(ctx, PSK_EHIP, "event wait failed");
                } else {
                    rc = chain_finalize(ctx, lane_of(i - 1));  // waits for chain i - 1: its upload is done too
                }
                t_final += t0.s();
                if (rc == PSK_OK && !q.consumer) report(i - 1);
                if (rc == PSK_OK && q.sketch_k) rc = collect_sketch(i - 1);
                release_upto(i);
            }
            // the sketch of sample i: queued behind its chain, collected one sample later (after chain i + 1 has been
            // queued, so the stream never runs dry; before sample i + 2 is uploaded into this lane's clean-stream buffer)
            if (rc == PSK_OK && q.sketch_k && wins[i] > 0)
                rc = sketch_enqueue(ctx, lane_of(i), lane_of(i).raw.as<uint8_t>(), clen[i], q.sketch_k, q.sketch_size, q.sketch_seed);
            // set (i + 2) % 3 is free again: chain i - 1 has been finalised and its sketch collected
            if (rc == PSK_OK && i + 2 < n) rc = stage_a(i + 2);
        }
        if (rc == PSK_OK && n > 0 && !q.consumer) {
            rc = chain_finalize(ctx, lane_of(n - 1));
            if (rc == PSK_OK) report(n - 1);
            if (rc == PSK_OK && q.sketch_k) rc = collect_sketch(n - 1);
        }
    }

    // nothing of this call may still be in flight when it returns (the ring and the caller's buffers)
    void sync_all()
    {
        const hipError_t e1 = hipStreamSynchronize(ctx->copy_stream ? ctx->copy_stream : ctx->stream);
        for (hipStream_t cs2 : ctx->copy_more) if (cs2) (void)hipStreamSynchronize(cs2);
        if (ctx->frame_stream) (void)hipStreamSynchronize(ctx->frame_stream);
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        if (ctx->sketch_stream) (void)hipStreamSynchronize(ctx->sketch_stream);
        if (rc == PSK_OK && (e1 != hipSuccess || e2 != hipSuccess))
            rc = psk_fail(ctx, PSK_EHIP, "stream synchronisation failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        for (CountLane &L : ctx->lane) L.sample = -1;
    }

    int run()
    {
        PSK_TRY(make_plan());
        start_workers();
        for (CountLane &L : ctx->lane) { L.sample = -1; L.sk_state = 0; }
        if (grouped()) rc = carve_lanes(ctx, NL, max_len, gpu_framing);
        t_setup = t_call.s();   // (PSK_TRACE: buffer sets carved, threads started)
        if (rc == PSK_OK) {
            if (grouped()) run_grouped();
            else run_one_by_one();
        }
        sync_all();   // before the workers are released: they write into the ring the uploads read
        release_upto(n);
        stop_workers();
        if (env_flag("PSK_TRACE"))
            fprintf(stderr, "[psk] count batch: %d samples %.1f ms; the caller waited %.1f ms for the host threads (their fills: %.1f ms "
                            "in all), %.1f ms for uploads + framing, %.1f ms for chains; set-up %.1f ms\n", n, t_call.s() * 1e3, t_worker * 1e3,
                    t_fill_us.load() / 1e3, t_frame * 1e3, t_final * 1e3, t_setup * 1e3);
        return rc;
    }
};

}  // namespace

int count_batch_core(psk_ctx *ctx, const CountRequest &q)
{
    if (!ctx) return PSK_EINVAL;
    if (q.sketch_k != 0) {
        if (q.sketch_k < 1 || q.sketch_k > 32 || q.sketch_size < 1) return psk_fail(ctx, PSK_EINVAL, "bad sketch parameters");
        if (!q.hashes_out || !q.n_hashes_out) return psk_fail(ctx, PSK_EINVAL, "null sketch buffers");
    }
    if (!q.consumer) {
        if (ctx->k == 0) return psk_fail(ctx, PSK_ESTATE, "psk_begin has not been called");
        if (q.n < 0 || q.first_sample_idx < 0 || q.first_sample_idx + q.n > ctx->n_samples)
            return psk_fail(ctx, PSK_EINVAL, "sample range out of bounds");
    }
    if (q.n == 0) return PSK_OK;
    if ((!q.bytes && !q.paths) || !q.lens) return psk_fail(ctx, PSK_EINVAL, "null input");
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    return BatchRun(ctx, q).run();
}

// one sample = a batch of one: the same framing (on the GPU for FASTA / four-line FASTQ) and the same chain
extern "C" int psk_count_kmers(psk_ctx *ctx, int sample_idx, const uint8_t *bytes, size_t len, uint64_t *n_unique,
                               uint64_t *n_total)
{
    if (!ctx) return PSK_EINVAL;
    if (ctx->k == 0) return psk_fail(ctx, PSK_ESTATE, "psk_begin has not been called");
    if (sample_idx < 0 || sample_idx >= ctx->n_samples) return psk_fail(ctx, PSK_EINVAL, "sample_idx out of range");
    if (!bytes && len) return psk_fail(ctx, PSK_EINVAL, "null input");
    static const uint8_t none = 0;
    const uint8_t *one = bytes ? bytes : &none;
    CountRequest q;
    q.first_sample_idx = sample_idx; q.n = 1; q.bytes = &one; q.lens = &len; q.n_unique = n_unique; q.n_total = n_total;
    return count_batch_impl(ctx, q);
}

// Batch form: `n_threads` host threads frame samples ahead into a ring of pinned buffers while the calling
// thread drives the GPU half of the samples in order, so host tokenisation overlaps device work.
extern "C" int psk_count_kmers_batch(psk_ctx *ctx, int first_sample_idx, int n, const uint8_t *const *bytes,
                                     const size_t *lens, uint64_t *n_unique, uint64_t *n_total, int n_threads)
{
    return psk_count_kmers_batch_sketch(ctx, first_sample_idx, n, bytes, lens, n_unique, n_total, n_threads, 0, 0, 0, nullptr,
                                        nullptr);
}

// Same, and (sketch_k > 0) the Mash-compatible MinHash sketch of every sample from the clean stream that is
// already on the device for counting -- the `-w` path needs both and the host frames each file once.
extern "C" int psk_count_kmers_batch_sketch(psk_ctx *ctx, int first_sample_idx, int n, const uint8_t *const *bytes,
                                            const size_t *lens, uint64_t *n_unique, uint64_t *n_total, int n_threads,
                                            int sketch_k, int sketch_size, uint32_t sketch_seed, uint64_t *hashes_out,
                                            uint64_t *n_hashes_out)
{
    CountRequest q;
    q.first_sample_idx = first_sample_idx; q.n = n; q.bytes = bytes; q.lens = lens; q.n_unique = n_unique; q.n_total = n_total;
    q.n_threads = n_threads; q.sketch_k = sketch_k; q.sketch_size = sketch_size; q.sketch_seed = sketch_seed;
    q.hashes_out = hashes_out; q.n_hashes_out = n_hashes_out;
    return count_batch_impl(ctx, q);
}

// The same for uncompressed files on disk: the framing threads read them, so no file image crosses the caller's
// language boundary (in Python: no bytes object per sample, no GIL hand-offs).
extern "C" int psk_count_kmers_files(psk_ctx *ctx, int first_sample_idx, int n, const char *const *paths, const size_t *sizes,
                                     uint64_t *n_unique, uint64_t *n_total, int n_threads, int sketch_k, int sketch_size,
                                     uint32_t sketch_seed, uint64_t *hashes_out, uint64_t *n_hashes_out)
{
    CountRequest q;
    q.first_sample_idx = first_sample_idx; q.n = n; q.paths = paths; q.lens = sizes; q.n_unique = n_unique; q.n_total = n_total;
    q.n_threads = n_threads; q.sketch_k = sketch_k; q.sketch_size = sketch_size; q.sketch_seed = sketch_seed;
    q.hashes_out = hashes_out; q.n_hashes_out = n_hashes_out;
    return count_batch_impl(ctx, q);
}
