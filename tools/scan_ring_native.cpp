// The two-in-flight scan ring of bench.py's run_steps without Python: psk_chi2_scan_begin / psk_scan_end on a matrix
// filled by psk_synth_presence (seed bits 48..63 = 80, as bench.py's matrix workload), medians of the host time inside
// begin and end and the wall-clock per step, as one JSON line.  Its difference to tools/scan_step_cost.py on a matrix of
// the same rows is the Python glue's share of a step.  (The encoder declines generated matrices -- presence_compact.hip --,
// so the ring's kernel is the dense chi2_scan_kernel; end_us holds the wait for it.)
//
//     make -C phenotypeseeker_amd/csrc scan_ring_native && tools/scan_ring_native [steps=4000] [rows=1048576] [samples=256]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "psk.h"

static double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static double median(std::vector<double> v, size_t skip)
{
    if (v.size() <= skip) return 0.0;
    v.erase(v.begin(), v.begin() + skip);
    std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
    return v[v.size() / 2];
}

#define CHECK(call)                                                                             \
    do {                                                                                        \
        const int rc_ = (call);                                                                 \
        if (rc_ != 0) {                                                                         \
            fprintf(stderr, "%s: %d (%s)\n", #call, rc_, ctx ? psk_last_error(ctx) : "no context"); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

int main(int argc, char **argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 4000;
    const uint64_t rows = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1ull << 20;
    const int n = argc > 3 ? atoi(argv[3]) : 256;
    if (steps < 4 || rows < 1 || n < 1) { fprintf(stderr, "usage: scan_ring_native [steps >= 4] [rows] [samples]\n"); return 2; }
    psk_ctx *ctx = nullptr;
    CHECK(psk_init(0, &ctx));
    CHECK(psk_begin(ctx, 13, n, 0, 0));
    CHECK(psk_synth_presence(ctx, rows, n, (80ull << 48) | 7ull));
    std::vector<int8_t> pheno(n);
    for (int i = 0; i < n; i++) pheno[i] = i % 2 == 0 ? 1 : 0;
    uint64_t npass = 0;
    double settle_ms = 0;
    CHECK(psk_chi2_scan(ctx, pheno.data(), nullptr, 2, n - 2, 0.05, 0, rows, &npass));
    CHECK(psk_rescan_timed(ctx, 300, &settle_ms));   // clocks settled, as bench.py does before its steps
    std::vector<double> begin_us, end_us, kernel_us;
    for (int i = 0; i < 2; i++) CHECK(psk_chi2_scan_begin(ctx, pheno.data(), nullptr, 2, n - 2, 0.05, 0, rows));
    const double t_loop = now_us();
    for (int i = 0; i < steps; i++) {
        double t0 = now_us();
        CHECK(psk_scan_end(ctx, &npass));
        end_us.push_back(now_us() - t0);
        kernel_us.push_back(psk_last_scan_ms(ctx) * 1e3);
        if (i + 2 < steps) {
            t0 = now_us();
            CHECK(psk_chi2_scan_begin(ctx, pheno.data(), nullptr, 2, n - 2, 0.05, 0, rows));
            begin_us.push_back(now_us() - t0);
        }
    }
    const double step_us = (now_us() - t_loop) / steps;
    const size_t skip = std::min<size_t>(begin_us.size() / 10, 100);   // the first steps: the queue is not in its steady state yet
    printf("{\"tool\": \"scan_ring_native\", \"rows\": %llu, \"samples\": %d, \"steps\": %d, \"survivors\": %llu, "
           "\"begin_us_p50\": %.3f, \"end_us_p50\": %.3f, \"step_us\": %.3f, \"kernel_us_p50\": %.3f}\n",
           (unsigned long long)rows, n, steps, (unsigned long long)npass, median(begin_us, skip), median(end_us, skip), step_us,
           median(kernel_us, skip));
    psk_free(ctx);
    return 0;
}
