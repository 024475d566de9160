// CPU check of csrc/stage_pipeline.h with stub stages (built and run by tests/test_stage_pipeline_host.py; needs no GPU).
// Every stage call logs a start and an end mark under one mutex, so the log is a total order.  For R runs: the three wait rules
// must hold in the log.  For a failure injected at every (stage, run): the pipeline returns that failure's code and text, nothing
// that depends on the failed stage (the same or a later stage of the same or a later run) ever started, and the program ends --
// the ending is what exercises the `failed_rc` term of wait_for: without it a thread waits for a counter that never moves.  What
// is NOT looked at: stages that do not depend on the failed one (a read or an inflate after a failed count).  The log has no
// mark for "the failure is published", and a thread that has passed its wait just before may rightly still start its stage,
// so "nothing starts after the failure" cannot be asserted from the log without a race in the check itself.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phenotypeseeker_amd/csrc/stage_pipeline.h"

namespace {

enum { READ = 0, INFLATE = 1, COUNT = 2 };
struct Mark { int stage, run; bool end; };

struct Harness {
    std::mutex log_m;
    std::vector<Mark> log;
    int fail_stage = -1, fail_run = -1;
    static thread_local std::string last_error;   // what psk_error_text would return on the failing thread

    void mark(int stage, int run, bool end)
    {
        std::lock_guard<std::mutex> lk(log_m);
        log.push_back({stage, run, end});
    }
    int stage(int s, int run)
    {
        mark(s, run, false);
        std::this_thread::sleep_for(std::chrono::microseconds(50 * ((s * 7 + run * 3) % 5)));   // uneven stages
        if (s == fail_stage && run == fail_run) {
            last_error = "stage " + std::to_string(s) + " of run " + std::to_string(run) + " failed";
            return 100 + 10 * s + run;   // (no end mark: the stage did not complete)
        }
        mark(s, run, true);
        return 0;
    }
    int position(int stage, int run, bool end) const
    {
        for (size_t i = 0; i < log.size(); i++)
            if (log[i].stage == stage && log[i].run == run && log[i].end == end) return (int)i;
        return -1;
    }
    int go(int R, std::string *why)
    {
        return StagePipeline().run(R, [&](int k) { return stage(READ, k); }, [&](int k) { return stage(INFLATE, k); },
                                   [&](int k) { return stage(COUNT, k); }, [] { return last_error; }, why);
    }
};
thread_local std::string Harness::last_error;

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            failures++;                                   \
            fprintf(stderr, "FAILED: %s: ", #cond);       \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

// start of (stage, run) lies after the end of (before_stage, before_run), where that run exists
void after(const Harness &h, int stage, int run, int before_stage, int before_run)
{
    if (before_run < 0) return;
    const int s = h.position(stage, run, false), e = h.position(before_stage, before_run, true);
    CHECK(s >= 0 && e >= 0 && e < s, "stage %d of run %d started at %d, stage %d of run %d ended at %d", stage, run, s, before_stage,
          before_run, e);
}

void check_waits(int R)
{
    Harness h;
    std::string why = "untouched";
    const int rc = h.go(R, &why);
    CHECK(rc == 0 && why == "untouched", "R = %d: rc %d", R, rc);
    CHECK((int)h.log.size() == 6 * R, "R = %d: %zu marks", R, h.log.size());
    for (int k = 0; k < R; k++) {
        after(h, READ, k, INFLATE, k - 2);
        after(h, INFLATE, k, READ, k);
        after(h, INFLATE, k, COUNT, k - 2);
        after(h, COUNT, k, INFLATE, k);
    }
}

void check_failure(int R, int fs, int fr)
{
    Harness h;
    h.fail_stage = fs;
    h.fail_run = fr;
    std::string why;
    const int rc = h.go(R, &why);
    CHECK(rc == 100 + 10 * fs + fr, "R = %d, failure at (%d, %d): rc %d", R, fs, fr, rc);
    CHECK(why == "stage " + std::to_string(fs) + " of run " + std::to_string(fr) + " failed", "R = %d, (%d, %d): text '%s'", R, fs, fr, why.c_str());
    // what depends on the failed stage never starts: the same or a later stage of the same or a later run
    for (const Mark &m : h.log)
        CHECK(!(m.stage >= fs && m.run >= fr && !(m.stage == fs && m.run == fr)), "R = %d, failure at (%d, %d): stage %d of run %d ran", R, fs,
              fr, m.stage, m.run);
    CHECK(h.position(fs, fr, true) < 0, "the failed stage has an end mark");
}

}  // namespace

int main()
{
    int points = 0;
    for (int rep = 0; rep < 20; rep++)
        for (int R : {1, 2, 3, 5}) {
            check_waits(R);
            points++;
            for (int fs = 0; fs < 3; fs++)
                for (int fr = 0; fr < R; fr++) {
                    check_failure(R, fs, fr);
                    points++;
                }
        }
    printf("stage pipeline check: %d runs, %d failures\n", points, failures);
    return failures ? 1 : 0;
}
