// xpbd_multi_frame.cpp -- a frame of the multi-GPU world (xpbd_multi.hpp): one shard's frame with its collectives, the frame on
// every local shard (the caller's thread or the workers), the end-of-frame check of the halos, undoing a frame, and
// xpbd_multi_world_step with its retry after a re-plan.
#include <algorithm>
#include <cmath>

#include "xpbd_multi.hpp"

namespace xpbd::multi {
namespace {

// One frame of local shard k and, behind it, the end-of-frame exchange: per rank the largest fraction of its travel allowance
// any owned body has used since the plan (squared) and the rank's status.  Enqueued by one thread per shard: the caller's
// with one local shard, worker k's with several (enqueue_frame).  The collectives, per thread:
//   RCCL   ncclAllGather on the shard's own communicator (one thread per device, no group call);
//   local  local_send | BARRIER | local_copy | BARRIER | local_release.
// A local error (job.st) skips the shard's remaining launches, the collectives still run; a collective that could not be
// enqueued (job.fatal) skips the shard's remaining collectives.  Every thread passes every barrier whatever went wrong, so
// nobody is left waiting.  (A ShardJobFn: `world` is the xpbd_multi_world.)
void shard_frame(void *world, size_t k, double dt, uint32_t substeps, ShardJob &job, Barrier &bar) noexcept
{
    xpbd_multi_world *mw = static_cast<xpbd_multi_world *>(world);
    Shard &s = mw->shards[k];
    const bool multi = mw->n_ranks > 1;
    const double h = dt / (double)substeps; // src/solver.rs:4
    LocalStatus &st = job.st;
    auto hip_keep = [&st](hipError_t e, const char *what) {
        if (e != hipSuccess)
            st.keep(set_error(XPBD_E_HIP, "%s failed: %s", what, hipGetErrorString(e)));
    };
    // one all-gather: `bytes` of every rank's buffer `send` into row rank of my buffer `recv`
    auto gather = [&](size_t bytes, DeviceBuffer Shard::*send, DeviceBuffer Shard::*recv, hipStream_t stream) {
        if (mw->transport == XPBD_TRANSPORT_RCCL) {
            if (job.fatal.ok())
                job.fatal.keep(rccl_all_gather(mw, s, (s.*send).ptr, (s.*recv).ptr, bytes, stream));
            return;
        }
        if (job.fatal.ok())
            job.fatal.keep(local_send(s, stream));
        bar.arrive_and_wait(); // every shard's send event has been recorded
        if (job.fatal.ok())
            job.fatal.keep(local_copy(mw, s, send, (s.*recv).ptr, bytes, stream));
        bar.arrive_and_wait(); // every shard's receive event has been recorded
        if (job.fatal.ok())
            job.fatal.keep(local_release(mw, s, stream));
    };
    st.keep(bind(s));
    if (multi && st.ok())
        st.keep(xpbd::frame_snapshot_save(s.world));
    if (st.ok())
        st.keep(xpbd::halo_frame_begin_enqueue(s.world, dt));
    const uint64_t t0 = now_ns();
    if (st.ok())
        st.keep(xpbd::halo_frame_begin_collect(s.world, h));
    job.ns_wait_broadphase = now_ns() - t0;
    const xpbd::HaloLists lists = s.lists();
    const size_t bytes = (size_t)mw->plan.rows_per_rank() * kDyn * 8;
    for (uint32_t q = 0; q < substeps; ++q) {
        const bool last = q + 1 == substeps;
        // 1. the narrowphase, then the boundary bodies: their end-of-substep state lands in the send buffer
        if (st.ok())
            st.keep(xpbd::halo_substep_boundary(s.world, h, q, last, lists));
        // 2. ONE all-gather per substep on the communication stream ...
        if (multi) {
            hip_keep(hipEventRecord(s.ev_ready, s.stream), "hipEventRecord");
            hip_keep(hipStreamWaitEvent(s.comm_stream, s.ev_ready, 0), "hipStreamWaitEvent");
            gather(bytes, &Shard::send, &Shard::recv, s.comm_stream);
            hip_keep(hipEventRecord(s.ev_gathered, s.comm_stream), "hipEventRecord");
        }
        // 3. ... while the interior bodies (nobody mirrors them) run on the world stream
        if (st.ok())
            st.keep(xpbd::halo_substep_interior(s.world, h, q, last, lists));
        // 4. the ghosts take their owners' state from the gathered buffer.  The next substep's boundary launch rewrites the
        // send buffer only after this exchange has read it: the communication stream is in order, so waiting for
        // ev_gathered covers the own copy; the peers' reads of OUR buffer are ordered by the transport (RCCL completes the
        // collective, local_release makes the communication stream wait for every peer's receive event).
        if (multi) {
            hip_keep(hipStreamWaitEvent(s.stream, s.ev_gathered, 0), "hipStreamWaitEvent");
            if (st.ok())
                st.keep(xpbd::halo_substep_ghosts(s.world, h, q, last, lists));
        }
    }
    if (multi) {
        // halo validity of THIS frame and the ranks' status, agreed on by all ranks
        hip_keep(hipMemsetAsync(s.disp.ptr, 0, 16, s.stream), "hipMemsetAsync");
        if (st.ok())
            st.keep(xpbd_world_max_displacement2(s.world, s.owned_slots.as<uint32_t>(), (uint32_t)s.held_ids.size(), s.snapshot.as<double>(),
                                                 s.disp_scale.as<double>(), s.disp.as<double>()));
        *s.status_host = (double)st.rc; // (after the last local launch that could still fail)
        hip_keep(hipMemcpyAsync(s.disp.as<double>() + 1, s.status_host, 8, hipMemcpyHostToDevice, s.stream), "hipMemcpyAsync");
        gather(16, &Shard::disp, &Shard::disp_all, s.stream);
        hip_keep(hipMemcpyAsync(s.disp_host, s.disp_all.ptr, (size_t)mw->n_ranks * 16, hipMemcpyDeviceToHost, s.stream), "hipMemcpyAsync");
    }
}

// Enqueues one whole frame on every local shard (shard_frame): on this thread with one local shard, on the workers with
// several.  Local errors are kept in `st` (the first in shard order); a collective that could not be enqueued breaks the
// transport.  Workers that cannot be started throw: the caller's handler breaks the world like any host failure of a step,
// remote ranks may already wait in this frame's collectives.
int enqueue_frame(xpbd_multi_world *mw, double dt, uint32_t substeps, LocalStatus &st)
{
    const uint64_t t0 = now_ns();
    ShardJob alone;
    const ShardJob *jobs = &alone;
    if (mw->shards.size() == 1) {
        Barrier bar; // one party: arrive_and_wait passes straight through
        shard_frame(mw, 0, dt, substeps, alone, bar);
    } else {
        mw->workers.run(mw->shards.size(), dt, substeps, shard_frame, mw);
        jobs = mw->workers.results();
    }
    uint64_t wait = 0;
    for (size_t k = 0; k < mw->shards.size(); ++k)
        wait = std::max(wait, jobs[k].ns_wait_broadphase);
    mw->timers.ns_wait_broadphase += wait;
    mw->timers.ns_enqueue += (now_ns() - t0) - wait;
    for (size_t k = 0; k < mw->shards.size(); ++k)
        if (!jobs[k].fatal.ok())
            return transport_broken(mw, jobs[k].fatal.report());
    for (size_t k = 0; k < mw->shards.size() && st.ok(); ++k)
        st = jobs[k].st;
    return XPBD_OK;
}

// Waits for the frame's last exchange.  *moved = the largest fraction of its travel allowance any owned body of any rank
// has used since the plan, in margin-equivalent metres (x halo_margin): a body next to a shard boundary may travel
// halo_margin, one more than two cells away from every foreign body halo_margin + half a cell edge (HaloPlanner::plan_rank).
// Returns the error all ranks agree on, if any rank had one.
int finish_frame(xpbd_multi_world *mw, LocalStatus &st, double *moved)
{
    const uint64_t t0 = now_ns();
    double worst = 0.0;
    int64_t peer_rc = 0;
    uint32_t peer = 0;
    for (Shard &s : mw->shards) {
        (void)hipSetDevice(s.device);
        const hipError_t e = hipStreamSynchronize(s.stream);
        if (e != hipSuccess)
            return transport_broken(mw, set_error(XPBD_E_HIP, "xpbd_multi_world_step: hipStreamSynchronize failed: %s", hipGetErrorString(e)));
        for (uint32_t r = 0; r < mw->n_ranks; ++r) {
            const double d = s.disp_host[2 * r], code = s.disp_host[2 * r + 1];
            if (d != d) // (the kernel already counts a NaN position as +inf)
                worst = INFINITY;
            else if (d > worst)
                worst = d;
            if (code != 0.0 && peer_rc == 0) {
                peer_rc = (int64_t)code;
                peer = r;
            }
        }
    }
    mw->timers.ns_wait_frame += now_ns() - t0;
    *moved = std::sqrt(worst) * mw->margin; // "margin-equivalent" metres: halo_margin means the allowance is used up
    if (!st.ok())
        return st.report();
    if (peer_rc != 0)
        return set_error((int)peer_rc, "xpbd_multi_world_step: rank %u failed with error %d in this frame (see its xpbd_last_error); the frame "
                                       "is undone on every rank", peer, (int)peer_rc);
    return XPBD_OK;
}

int restore_frame(xpbd_multi_world *mw)
{
    for (Shard &s : mw->shards)
        XPBD_TRY(xpbd::frame_snapshot_restore(s.world));
    return XPBD_OK;
}

} // namespace
} // namespace xpbd::multi

using namespace xpbd::multi;

extern "C" {

int xpbd_multi_world_step(xpbd_multi_world *mw, double dt, uint32_t substeps)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_step"));
    WorldReport::StepGuard report_guard(mw->report);
    PlanState &plan = mw->plan;
    if (substeps == 0)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_step: substeps must be > 0");
    if (!plan.planned)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_step: no bodies uploaded");
    if (plan.violated)
        return set_error(XPBD_E_HALO, "xpbd_multi_world_step: a body used up its travel allowance within the last frame (%.3g m in margin-equivalent "
                                      "metres, halo_margin %.3g m); that frame was undone -- call xpbd_multi_world_replan (and re-plan more often "
                                      "or raise the margin)", plan.last_displacement, mw->margin);
    ++mw->timers.steps;
    for (int attempt = 0;; ++attempt) {
        LocalStatus st;
        XPBD_TRY(enqueue_frame(mw, dt, substeps, st));
        if (mw->n_ranks == 1) { // no ghosts, nothing to validate: asynchronous after the broadphase (unless reports are gathered)
            if (!st.ok())
                return st.report();
            return mw->report.on ? capture_report(mw) : XPBD_OK;
        }
        double moved = 0.0;
        if (int rc = finish_frame(mw, st, &moved)) {
            if (mw->broken)
                return rc;
            LocalStatus failed;
            failed.keep(rc);
            (void)restore_frame(mw); // best effort: the state of the frame's start, on every rank
            return failed.report();
        }
        const double gain = std::max(0.0, moved - plan.last_displacement); // what this frame used up of the allowance
        plan.frame_moved(moved);
        if (moved <= mw->margin) {
            if (mw->report.on) // before a re-plan repacks the shards
                XPBD_TRY(capture_report(mw));
            // pre-emptive: another frame like this one (and half as much again) would outrun the allowance, so re-plan (and
            // re-balance) from the state just reached.  A wrong guess costs a frame: it is undone and run again below.
            if ((mw->flags & XPBD_MULTI_AUTO_REPLAN) && moved + 1.5 * gain > mw->margin)
                XPBD_TRY(replan(mw));
            return XPBD_OK;
        }
        // A body outran its allowance during THIS frame: a remote contact may have been missed in it.  Undo the frame.
        XPBD_TRY(restore_frame(mw));
        ++mw->timers.rollbacks;
        if (!(mw->flags & XPBD_MULTI_AUTO_REPLAN) || attempt == 1) {
            plan.violate();
            return set_error(XPBD_E_HALO, "xpbd_multi_world_step: a body used up its travel allowance during this frame (%.3g m in "
                                          "margin-equivalent metres, beyond halo_margin %.3g m%s): remote contacts may have been missed, so the "
                                          "frame was undone -- call xpbd_multi_world_replan and step again%s",
                             moved, mw->margin, attempt ? ", even right after a re-plan" : "",
                             attempt ? " with a larger halo_margin or a shorter frame" : "");
        }
        XPBD_TRY(replan(mw)); // from the restored state; then the same frame again
    }
} XPBD_MULTI_ABI_CATCH

} // extern "C"
