// a1: the batch as the entry points hand it over.  Samples that are gzip images (magic bytes; glistmaker reads .gz through zlib:
// SURVEY.md section 2 row 9) are inflated on the device first (gz_inflate.hip) -- every .gz sample of a run in one go, runs
// cut where the text would pass PSK_GZ_GROUP_MB (8 GiB -- r06; ~1.5 GB of compressed input, 65,536 decoding lanes of 23 KB each: with r05's 12 GiB the inflate's buffers were 70 GB, and what a hipMalloc beyond the first ~40 GB of a process costs on this pool -- 20-30 ms per GB, tools/free_probe.py -- made 64 read sets take 2.1 s to the .pkl where 8-GiB runs take 1.27, 6-GiB 1.4, 4-GiB 1.56: profiles/r06_cfg5gz_groups.json) -- and their chains then start from text that is already in device
// memory; a member the device route declines has been inflated by zlib on the host and goes on as an in-memory sample.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>

#include "count_plan.h"
#include "gz_plan.h"
#include "psk_internal.h"
#include "stage_pipeline.h"

static_assert(PSK_OK == 0, "StagePipeline takes 0 for success");

int read_exact(const char *path, long offset, size_t len, void *dst)
{
    FILE *f = fopen(path, "rb");
    if (!f) return -1;
    size_t got = 0;
    if (offset == 0 || fseek(f, offset, offset < 0 ? SEEK_END : SEEK_SET) == 0)
        while (got < len) {
            const size_t r = fread(static_cast<uint8_t *>(dst) + got, 1, len - got, f);
            if (r == 0) break;
            got += r;
        }
    fclose(f);
    return got == len ? 0 : -1;
}

namespace {

// The .gz runs of one call.  A run's images are read (by the threads the framing would use) and inflated into buffer set
// `set`; its chains then start from text in device memory: eb / ep / el / gs are the call's inputs as count_batch_core sees them.
struct GzRuns {
    struct Run : psk_gz_run_cut {
        std::vector<size_t> sizes;       // its .gz samples' images' sizes, where they lie in the device buffer
        std::vector<uint64_t> at;
        bool on_device = false;          // the device inflates them (else: zlib on host threads)
        std::vector<GzInflated> res;
        double ms_read = 0;
    };
    psk_ctx *ctx;
    const CountRequest &q;
    const int n;
    const bool host_only = env_flag("PSK_HOST_FRAMING");   // (the A/B knob of the host's state machine: the host's inflate with it)
    const bool trace = env_flag("PSK_TRACE");
    std::vector<uint8_t *> held;   // where the compressed image of a .gz FILE is (a mapping, or a slice of ctx->gz_host[set])
    std::vector<const uint8_t *> eb;
    std::vector<const char *> ep;
    std::vector<size_t> el;
    std::vector<GzSample> gs;
    std::vector<Run> runs;
    Stopwatch t_all;

    GzRuns(psk_ctx *c, const CountRequest &req) : ctx(c), q(req), n(req.n), held(n, nullptr), eb(n, nullptr), ep(n, nullptr), el(n, 0), gs(n) {}
    bool in_memory(int i) const { return q.bytes && q.bytes[i]; }
    const uint8_t *image(int i) const { return in_memory(i) ? q.bytes[i] : held[(size_t)i]; }

    // ISIZE of the last member (the text of a one-member file, modulo 2^32) is what a run's budget is counted in
    void cut(const std::vector<char> &is_gz, size_t budget)
    {
        std::vector<size_t> isize((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            if (!is_gz[(size_t)i]) continue;
            uint8_t d[4] = {0, 0, 0, 0};
            if (in_memory(i)) memcpy(d, q.bytes[i] + q.lens[i] - 4, 4);
            else if (read_exact(q.paths[i], -4, 4, d) != 0) memset(d, 0, 4);
            isize[(size_t)i] = (size_t)d[0] | ((size_t)d[1] << 8) | ((size_t)d[2] << 16) | ((size_t)d[3] << 24);
        }
        for (psk_gz_run_cut &c : psk_cut_gz_runs(n, is_gz.data(), q.lens, isize.data(), budget)) {
            runs.emplace_back();
            static_cast<psk_gz_run_cut &>(runs.back()) = std::move(c);
        }
    }

    // (up != nullptr: the device buffer of the run's images; file j of the run goes to up + r.at[j] as soon as it has been read)
    int read_images(Run &r, uint8_t *up)
    {
        // r06: a .gz FILE is not read into host memory of the library's own any more -- it is MAPPED (read-only, private), the upload
        // copies out of the mapping (the page cache's pages: no fresh anonymous pages to fault in, 0.3 s per 2 GB), and what the host
        // itself reads of an image -- member headers, trailers, the whole of a file the device declines -- it reads there too.  Giving 5.2 GB
        // of such buffers back cost psk_build_presence 0.5 s of cfg5gz's 2.3 s (on a helper thread the same half second was spent by
        // whoever next touched the address space); an unmapped file gives no page back.  PSK_GZ_READ=1: r05's buffers (and what a
        // file that cannot be mapped gets).
        const bool map_files = !env_flag("PSK_GZ_READ");
        const size_t *lens = q.lens;
        std::vector<std::pair<void *, size_t>> &maps = ctx->gz_maps[r.set];
        for (auto &m : maps) munmap(m.first, m.second);   // (the run before last of this set: inflated and counted)
        maps.clear();
        size_t need = 0;
        std::vector<char> mapped((size_t)n, 0);
        for (int i : r.idx) {
            if (in_memory(i)) continue;
            if (map_files && lens[i]) {
                const int fd = open(q.paths[i], O_RDONLY | O_CLOEXEC);
                struct stat sb;
                void *m = MAP_FAILED;
                if (fd >= 0 && fstat(fd, &sb) == 0 && (size_t)sb.st_size >= lens[i]) m = mmap(nullptr, lens[i], PROT_READ, MAP_PRIVATE, fd, 0);
                if (fd >= 0) close(fd);
                if (m != MAP_FAILED) {
                    (void)madvise(m, lens[i], MADV_SEQUENTIAL);
                    maps.push_back({m, lens[i]});
                    held[(size_t)i] = static_cast<uint8_t *>(m);
                    mapped[(size_t)i] = 1;
                    continue;
                }
            }
            need += (lens[i] + 63) & ~(size_t)63;
        }
        uint8_t *&host = ctx->gz_host[r.set];
        size_t &cap = ctx->gz_host_cap[r.set];
        if (need > cap) {
            if (ctx->gz_reaper.joinable()) ctx->gz_reaper.join();
            std::free(host);
            cap = 0;
            host = static_cast<uint8_t *>(std::malloc(need + need / 8));
            if (!host) return psk_fail(ctx, PSK_ENOMEM, "no host memory for %zu bytes of compressed input", need);
            cap = need + need / 8;
        }
        size_t used = 0;
        for (int i : r.idx)
            if (!in_memory(i) && !mapped[(size_t)i]) {
                held[(size_t)i] = host + used;
                used += (lens[i] + 63) & ~(size_t)63;
            }
        std::atomic<int> next(0), failed(-1), up_failed(0);
        auto reader = [&]() {
            if (up && hipSetDevice(ctx->device) != hipSuccess) up_failed = 1;
            for (;;) {
                const int j = next.fetch_add(1);
                if (j >= (int)r.idx.size()) return;
                const int i = r.idx[(size_t)j];
                if (!in_memory(i) && !mapped[(size_t)i] && read_exact(q.paths[i], 0, lens[i], held[(size_t)i]) != 0) {
                    failed = i;
                    continue;
                }
                if (up && lens[i] && hipMemcpyAsync(up + r.at[j], image(i), lens[i], hipMemcpyHostToDevice, ctx->gz_up_stream) != hipSuccess) up_failed = 1;
            }
        };
        std::vector<std::thread> pool;
        const int nt = q.n_threads < 1 ? 1 : (q.n_threads > 16 ? 16 : q.n_threads);
        for (int t = 1; t < nt && t < (int)r.idx.size(); t++) pool.emplace_back(reader);
        reader();
        for (auto &t : pool) t.join();
        if (failed >= 0) return psk_fail(ctx, PSK_ERANGE, "reading sample %d (%s) failed", q.first_sample_idx + failed.load(), q.paths[failed.load()]);
        if (up_failed) return psk_fail(ctx, PSK_EHIP, "uploading the compressed images failed");
        return PSK_OK;
    }

    // stage 1 of a run: its images read (and, for a run the device inflates, uploaded as they arrive, on a stream of their own)
    int stage_read(int k)
    {
        Run &r = runs[(size_t)k];
        for (int i = r.lo; i < r.hi; i++) {
            eb[(size_t)i] = q.bytes ? q.bytes[i] : nullptr;
            ep[(size_t)i] = q.paths ? q.paths[i] : nullptr;
            el[(size_t)i] = q.lens[i];
            gs[(size_t)i] = GzSample();
        }
        if (r.idx.empty()) return PSK_OK;
        PSK_HIP(ctx, hipSetDevice(ctx->device));
        const Stopwatch t0;
        for (int i : r.idx) r.sizes.push_back(q.lens[i]);
        PSK_TRY(gz_group_on_device(ctx, (int)r.idx.size(), r.sizes.data(), host_only, q.n_threads, &r.on_device));
        r.at.resize(r.idx.size());
        if (r.on_device) {
            const uint64_t total = gz_image_layout((int)r.idx.size(), r.sizes.data(), r.at.data());
            PSK_TRY(dev_reserve(ctx, ctx->gz_comp[r.set], total));
            PSK_HIP(ctx, hipMemsetAsync(ctx->gz_comp[r.set].p, 0, total, ctx->gz_up_stream));
        }
        PSK_TRY(read_images(r, r.on_device ? ctx->gz_comp[r.set].as<uint8_t>() : nullptr));
        if (r.on_device) PSK_HIP(ctx, hipStreamSynchronize(ctx->gz_up_stream));
        r.ms_read = t0.s() * 1e3;
        return PSK_OK;
    }

    // stage 2: inflated, and where each sample's records are
    int stage_inflate(int k)
    {
        Run &r = runs[(size_t)k];
        if (r.idx.empty()) return PSK_OK;
        PSK_HIP(ctx, hipSetDevice(ctx->device));
        const Stopwatch t1;
        std::vector<const uint8_t *> ptrs;
        for (int i : r.idx) ptrs.push_back(image(i));
        DevBuf &out = ctx->gz_out[r.set];
        PSK_TRY(gz_inflate_group(ctx, (int)r.idx.size(), ptrs.data(), r.sizes.data(), ctx->gz_comp[r.set], ctx->gz_sym, ctx->gz_rec, out, ctx->gz_tab, r.res, nullptr,
                                 host_only, q.n_threads, ctx->gz_stream, r.on_device));
        std::vector<uint8_t> head;
        for (size_t j = 0; j < r.idx.size(); j++) {
            const int i = r.idx[j];
            GzInflated &g = r.res[j];
            ep[(size_t)i] = nullptr;
            if (g.on_device) {
                // where the records start decides the format (frame_probe): the first bytes of the text come back for that
                const uint8_t *text = out.as<uint8_t>() + g.off;
                const size_t end = g.first_nul < g.len ? g.first_nul : g.len, look = end < 65536 ? end : 65536;
                head.resize(look + 1);
                if (look) {
                    PSK_HIP(ctx, hipMemcpyAsync(head.data(), text, look, hipMemcpyDeviceToHost, ctx->gz_stream));
                    PSK_HIP(ctx, hipStreamSynchronize(ctx->gz_stream));
                }
                size_t st = 0, en = 0;
                const int f = frame_probe_known_end(head.data(), look, &st, &en);
                if (f || look == end) {
                    gs[(size_t)i].dev = text;
                    gs[(size_t)i].fmt = f;
                    gs[(size_t)i].roff = f ? st : end;
                    gs[(size_t)i].rlen = f ? end - st : 0;
                    eb[(size_t)i] = nullptr;
                    el[(size_t)i] = g.len;
                    continue;
                }
                // no record in the first 64 KB: the whole text comes back and takes the in-memory route
                g.host.resize(g.len);
                PSK_HIP(ctx, hipMemcpyAsync(g.host.data(), text, g.len, hipMemcpyDeviceToHost, ctx->gz_stream));
                PSK_HIP(ctx, hipStreamSynchronize(ctx->gz_stream));
                g.on_device = false;
            }
            eb[(size_t)i] = g.host.data();
            el[(size_t)i] = g.host.size();
        }
        if (trace) {
            size_t text = 0, comp = 0;
            for (size_t j = 0; j < r.idx.size(); j++) {
                text += r.res[j].len;
                comp += r.sizes[j];
            }
            fprintf(stderr, "[psk] count batch: samples %d..%d: %zu .gz ones, %.1f MB read in %.1f ms, -> %.1f MB of text in %.1f ms\n", r.lo, r.hi - 1,
                    r.idx.size(), comp / 1e6, r.ms_read, text / 1e6, t1.s() * 1e3);
        }
        return PSK_OK;
    }

    // stage 3: the run's samples counted, its .gz ones from text in device memory
    int stage_count(int k)
    {
        const Run &r = runs[(size_t)k];
        const Stopwatch t_core;
        CountRequest in = q;
        in.bytes = eb.data(); in.paths = ep.data(); in.lens = el.data(); in.gzs = gs.data();
        const int rc = count_batch_core(ctx, in.slice(r.lo, r.hi - r.lo));
        if (trace)
            fprintf(stderr, "[psk] count batch: samples %d..%d counted in %.1f ms; %.1f ms since the call began\n", r.lo, r.hi - 1,
                    t_core.s() * 1e3, t_all.s() * 1e3);
        return rc;
    }

    // The three stages as a pipeline over the runs (stage_pipeline.h): run k + 2 is read while run k + 1 is inflated while run k is
    // counted -- a thread for each of the first two stages, the calling thread counts.  One run, or PSK_GZ_NO_LOOKAHEAD: in turn.
    int run_all()
    {
        const int R = (int)runs.size();
        t_all = Stopwatch();
        if (R == 1 || env_flag("PSK_GZ_NO_LOOKAHEAD")) {
            for (int k = 0; k < R; k++) {
                PSK_TRY(stage_read(k));
                PSK_TRY(stage_inflate(k));
                PSK_TRY(stage_count(k));
            }
            return PSK_OK;
        }
        std::string why;
        const int rc = StagePipeline().run(R, [this](int k) { return stage_read(k); }, [this](int k) { return stage_inflate(k); },
                                           [this](int k) { return stage_count(k); }, [this] { return psk_error_text(ctx); }, &why);
        if (rc != PSK_OK) psk_set_error_text(ctx, why);
        return rc;
    }
};

}  // namespace

int count_batch_impl(psk_ctx *ctx, const CountRequest &q)
{
    const int n = q.n;
    if (!ctx || n <= 0 || (!q.bytes && !q.paths) || !q.lens || env_flag("PSK_NO_GPU_GZ")) return count_batch_core(ctx, q);
    std::vector<char> is_gz((size_t)n, 0);
    bool any = false;
    for (int i = 0; i < n; i++) {
        uint8_t m[2] = {0, 0};
        if (q.lens[i] < 18) continue;
        if (q.bytes && q.bytes[i]) memcpy(m, q.bytes[i], 2);
        else if (q.paths && q.paths[i] && read_exact(q.paths[i], 0, 2, m) != 0) m[0] = 0;
        is_gz[(size_t)i] = m[0] == 0x1f && m[1] == 0x8b;
        any = any || is_gz[(size_t)i];
    }
    if (!any) return count_batch_core(ctx, q);
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->gz_stream) PSK_HIP(ctx, hipStreamCreateWithFlags(&ctx->gz_stream, hipStreamNonBlocking));
    if (!ctx->gz_up_stream) PSK_HIP(ctx, hipStreamCreateWithFlags(&ctx->gz_up_stream, hipStreamNonBlocking));
    size_t budget_mb = 8192;
    PSK_TRY(env_int(ctx, "PSK_GZ_GROUP_MB", 0, 1 << 30, &budget_mb));
    GzRuns g(ctx, q);
    g.cut(is_gz, budget_mb << 20);
    return g.run_all();
}
