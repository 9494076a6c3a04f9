// xpbd_multi_workers.hpp -- the host threads of the multi-GPU world's frame: the barrier they meet at, a collective operation's
// local status, a shard's result of a frame, and the pool that runs one job per local shard.  Host only (the standard library,
// xpbd_error.h and the codes of include/xpbd.h): tests/test_multi_workers_standalone.py builds it with plain g++.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/xpbd.h"
#include "xpbd_error.h"

#pragma GCC visibility push(hidden)

namespace xpbd::multi {

// One host thread per local shard (a process that owns several GPUs): a frame is ~20 runtime calls per shard and substep, and
// a single thread enqueueing them for 8 GPUs takes longer than the GPUs need to run them (measured on one device with four
// shards: 5.5 ms of enqueueing per 4.4 ms frame, profiles/r03_a_multi_host_time.json).  The threads meet at a barrier only
// where the in-process transport needs every shard's event to have been RECORDED before anybody waits for it.
struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    uint32_t n = 1, waiting = 0;
    uint64_t generation = 0;
    void arrive_and_wait() noexcept
    {
        std::unique_lock<std::mutex> lock(m);
        const uint64_t g = generation;
        if (++waiting == n) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g; });
        }
    }
};

// The first local error of a collective operation (a plan, a frame).  The operation goes on taking part in its collectives
// -- with whatever payload -- so that the ranks stay in step, and every collective carries each rank's status: all ranks
// leave the operation with an error at the same point.
struct LocalStatus {
    int rc = XPBD_OK;
    char message[xpbd::kErrorBytes] = {};
    void keep(int r) noexcept
    {
        if (rc == XPBD_OK && r != XPBD_OK) {
            rc = r;
            std::memcpy(message, xpbd_last_error(), sizeof message);
        }
    }
    bool ok() const { return rc == XPBD_OK; }
    int report() const noexcept { return set_error(rc, "%s", message); }
};

struct ShardJob {
    LocalStatus st;    // first local error of the shard's frame
    LocalStatus fatal; // first collective that could not be enqueued
    uint64_t ns_wait_broadphase = 0;
};

// What worker k does with one job: `ctx` is the caller's, job its own slot, bar the pool's barrier of n parties.  It passes
// every barrier whatever goes wrong, so nobody is left waiting.
using ShardJobFn = void (*)(void *ctx, size_t k, double dt, uint32_t substeps, ShardJob &job, Barrier &bar) noexcept;

// One enqueueing thread per local shard, started by the first run() and joined by the destructor.  Not started, the pool
// holds no thread and no result.
class FrameWorkers {
public:
    FrameWorkers() = default;
    FrameWorkers(const FrameWorkers &) = delete;
    FrameWorkers &operator=(const FrameWorkers &) = delete;
    ~FrameWorkers() { stop(); }

    // Runs fn(ctx, k, dt, substeps, ...) on worker k of n (the first call starts them; n stays what it was then) and returns when
    // every worker is through with it.  Workers that cannot all be started are stopped again -- the pool is as it was before
    // the call -- and the exception goes on to the caller.
    void run(size_t n, double dt, uint32_t substeps, ShardJobFn fn, void *ctx)
    {
        if (threads.empty()) {
            try {
                result.resize(n);
                barrier.n = (uint32_t)n;
                for (size_t k = 0; k < n; ++k)
                    threads.emplace_back(&FrameWorkers::worker_main, this, k);
            } catch (...) {
                stop();
                throw;
            }
        }
        std::unique_lock<std::mutex> lock(m);
        this->fn = fn, this->ctx = ctx, this->dt = dt, this->substeps = substeps, done = 0;
        ++job;
        cv_job.notify_all();
        cv_done.wait(lock, [&] { return done == (uint32_t)threads.size(); });
    }
    // results()[k]: what worker k left of the last job.
    const ShardJob *results() const { return result.data(); }

private:
    void worker_main(size_t k)
    {
        uint64_t seen = 0;
        for (;;) {
            ShardJobFn f;
            void *c;
            double t;
            uint32_t s;
            {
                std::unique_lock<std::mutex> lock(m);
                cv_job.wait(lock, [&] { return quit || job != seen; });
                if (quit)
                    return;
                seen = job;
                f = fn, c = ctx, t = dt, s = substeps;
            }
            result[k] = ShardJob();
            f(c, k, t, s, result[k], barrier);
            {
                std::lock_guard<std::mutex> lock(m);
                ++done;
            }
            cv_done.notify_one();
        }
    }
    void stop() noexcept
    {
        {
            std::lock_guard<std::mutex> lock(m);
            quit = true;
        }
        cv_job.notify_all();
        for (std::thread &t : threads)
            t.join();
        threads.clear();
        result.clear();
        quit = false;
        job = 0; // (a worker starts having seen job 0)
    }

    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    uint64_t job = 0;
    uint32_t done = 0;
    bool quit = false;
    ShardJobFn fn = nullptr;
    void *ctx = nullptr;
    double dt = 0.0;
    uint32_t substeps = 0;
    std::vector<ShardJob> result;
    Barrier barrier;
};

} // namespace xpbd::multi

#pragma GCC visibility pop
