// The frame workers of the multi-GPU world (csrc/xpbd_multi_workers.hpp) without a device: see test_multi_workers_standalone.py.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "../constraint_solver_amd/csrc/xpbd_multi_workers.hpp"

using namespace xpbd::multi;

namespace {

constexpr uint64_t kJobs = 200;

struct Context {
    uint64_t job = 0;                  // written by main before run(), read by the workers
    std::atomic<uint64_t> finished{0}; // jobs the workers are through with, over all jobs
};

double dt_of(uint64_t job) { return 0.25 * (double)job; }
uint32_t substeps_of(uint64_t job) { return (uint32_t)(job % 7 + 1); }
uint64_t stamp(uint64_t job, size_t k) { return job * 64 + k; }

// As shard_frame with the in-process transport: two barriers per job whatever went wrong, the slot written last.
void job_fn(void *ctx, size_t k, double dt, uint32_t substeps, ShardJob &job, Barrier &bar) noexcept
{
    Context &c = *static_cast<Context *>(ctx);
    if (dt != dt_of(c.job) || substeps != substeps_of(c.job))
        job.fatal.keep(xpbd::set_error(XPBD_E_INVALID, "job %llu worker %zu: wrong arguments", (unsigned long long)c.job, k));
    bar.arrive_and_wait();
    if (k == 1 && c.job % 3 == 0)
        job.st.keep(xpbd::set_error(XPBD_E_HALO, "job %llu worker %zu", (unsigned long long)c.job, k));
    bar.arrive_and_wait();
    job.ns_wait_broadphase = stamp(c.job, k);
    c.finished.fetch_add(1);
}

int fail(const char *what, size_t n, uint64_t job)
{
    std::fprintf(stdout, "FAILED: %s (pool of %zu, job %llu)\n", what, n, (unsigned long long)job);
    return 1;
}

int run_pool(size_t n)
{
    Context c;
    FrameWorkers pool;
    for (uint64_t job = 1; job <= kJobs; ++job) {
        c.job = job;
        pool.run(n, dt_of(job), substeps_of(job), job_fn, &c);
        // run() is back: every worker is through with THIS job and has written its slot
        if (c.finished.load() != job * n)
            return fail("run returned before every worker was through", n, job);
        const ShardJob *jobs = pool.results();
        const bool failing = n > 1 && job % 3 == 0;
        for (size_t k = 0; k < n; ++k) {
            if (jobs[k].ns_wait_broadphase != stamp(job, k))
                return fail("a slot does not hold (job, k)", n, job);
            if (!jobs[k].fatal.ok())
                return fail("a worker saw wrong arguments", n, job);
            if (jobs[k].st.ok() != !(failing && k == 1))
                return fail("an error in the wrong slot", n, job);
        }
        // the first error in shard order is the one reported (enqueue_frame's loop)
        LocalStatus st;
        for (size_t k = 0; k < n && st.ok(); ++k)
            st = jobs[k].st;
        if (st.ok() == failing)
            return fail("the error was not found", n, job);
        if (failing) {
            char expected[64];
            std::snprintf(expected, sizeof expected, "job %llu worker 1", (unsigned long long)job);
            (void)xpbd::set_error(XPBD_OK, "nothing");
            if (st.report() != XPBD_E_HALO || std::strcmp(xpbd_last_error(), expected) != 0)
                return fail("the reported error is not worker 1's", n, job);
        }
    }
    return 0; // (the pool goes right after a job)
}

} // namespace

int main()
{
    {
        FrameWorkers never_ran;
    }
    size_t pools = 0;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)8}) {
        if (run_pool(n))
            return 1;
        ++pools;
    }
    {
        Context c;
        c.job = 1;
        FrameWorkers once;
        once.run(4, dt_of(1), substeps_of(1), job_fn, &c);
    }
    std::printf("%zu pools ok\n", pools);
    return 0;
}
