// Three stages over R runs as a pipeline of three threads: run k + 2 is read while run k + 1 is inflated while run k is counted,
// on two buffer sets (run k's are run k - 2's).  Knows nothing of what the stages do (count_gz.hip: the .gz runs of a call), so it
// can be exercised on a CPU (tests/stage_pipeline_check.cpp).  The waits:
//   read of run k      after inflate of run k - 2    (the images of run k - 2 have been used)
//   inflate of run k   after read of run k and count of run k - 2   (the text of run k - 2 has been counted)
//   count of run k     after inflate of run k
// The first stage that fails makes the call: its code is returned, its text (run()'s error_text(), asked for on the failing thread
// before anyone else can fail) lands in *why; the other threads stop at their next wait.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

namespace {

struct StagePipeline {
    typedef std::function<int(int)> Stage;   // int(int run): 0 on success
    std::mutex m;
    std::condition_variable cv;
    int read_done = 0, inflate_done = 0, count_done = 0, failed_rc = 0;
    std::string failed_why;

    void fail(int rc, const std::function<std::string()> &error_text)
    {
        std::lock_guard<std::mutex> lk(m);
        if (failed_rc == 0) {
            failed_rc = rc;
            failed_why = error_text();
        }
        cv.notify_all();
    }
    bool wait_for(const int &counter, int at_least)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return failed_rc != 0 || counter >= at_least; });
        return failed_rc == 0;
    }
    void advance(int &counter)
    {
        std::lock_guard<std::mutex> lk(m);
        counter++;
        cv.notify_all();
    }

    // the calling thread counts; returns 0 or the first failure's code (*why: its text)
    int run(int R, const Stage &stage_read, const Stage &stage_inflate, const Stage &stage_count,
            const std::function<std::string()> &error_text, std::string *why)
    {
        // a thread's loop over the runs: stage k after `ready(k)`, then `done` moves on; it stops when anyone has failed
        auto drive = [&](const Stage &stage, int &done, auto ready) {
            for (int k = 0; k < R; k++) {
                if (!ready(k)) return;
                const int rc = stage(k);
                if (rc != 0) return fail(rc, error_text);
                advance(done);
            }
        };
        std::thread reader([&] { drive(stage_read, read_done, [&](int k) { return wait_for(inflate_done, k - 1); }); });
        std::thread inflater([&] { drive(stage_inflate, inflate_done, [&](int k) { return wait_for(read_done, k + 1) && wait_for(count_done, k - 1); }); });
        drive(stage_count, count_done, [&](int k) { return wait_for(inflate_done, k + 1); });
        reader.join();
        inflater.join();
        if (failed_rc != 0 && why) *why = failed_why;
        return failed_rc;
    }
};

}  // namespace
