// xpbd_multi_transport.cpp -- the transport of the multi-GPU world (xpbd_multi.hpp): one all-gather over all ranks, by RCCL or by
// peer copies inside the process, per shard (the frame) and for every local shard at once (plan time); the plan-time all-gather
// of host data with every rank's status; and what a collective that could not be enqueued does to the world.
#include <cstring>
#include <vector>

#include "xpbd_multi.hpp"

namespace xpbd::multi {

int bind(const Shard &s)
{
    XPBD_HIP_TRY(hipSetDevice(s.device));
    return XPBD_OK;
}

int nccl_fail(const xpbd_multi_world *mw, ncclResult_t r, const char *what)
{
    return set_error(XPBD_E_HIP, "%s failed: %s (RCCL from %s)", what, mw->rccl ? mw->rccl->GetErrorString(r) : "?", mw->rccl ? mw->rccl->path : "?");
}

// A collective that could not be enqueued leaves the ranks out of step for good: the communicators are aborted (peers
// blocked in the collective return with an error instead of hanging) and every later call on this world fails.
int transport_broken(xpbd_multi_world *mw, int rc) noexcept
{
    mw->broken = true;
    if (mw->rccl && mw->rccl->CommAbort)
        for (Shard &s : mw->shards)
            if (s.comm) {
                (void)hipSetDevice(s.device);
                (void)mw->rccl->CommAbort(s.comm);
                s.comm = nullptr;
            }
    return set_error(rc, "%s -- the communicator is unusable now: destroy this xpbd_multi_world on every rank", xpbd_last_error());
}

// ---- one all-gather over all ranks: every shard contributes `bytes` of its buffer `send` and receives n_ranks x bytes, row
// r from rank r, into its buffer `recv`.  Written per shard: all_gather_device_raw drives every local shard from one thread,
// shard_frame drives one shard from that shard's thread.

// RCCL: shard s's part of the collective, on `stream`.
int rccl_all_gather(xpbd_multi_world *mw, Shard &s, const void *send, void *recv, size_t bytes, hipStream_t stream)
{
    // RCCL reads the thread's last HIP error after its own calls: a stale, harmless one left by somebody else in the
    // process (hipErrorNotReady from an event query, say) would be reported as "unhandled cuda error"
    (void)hipGetLastError();
    const ncclResult_t r = mw->rccl->AllGather(send, recv, bytes, ncclChar, s.comm, stream);
    return r == ncclSuccess ? XPBD_OK : nccl_fail(mw, r, "ncclAllGather");
}

// XPBD_TRANSPORT_LOCAL (every rank lives in this process): peer copies ordered by events, in three phases.  Every shard's
// phase must have been enqueued before any shard enters the next one: a stream can only wait for an event already RECORDED.
// 1. my send buffer is ready
int local_send(Shard &s, hipStream_t stream)
{
    XPBD_HIP_TRY(hipEventRecord(s.ev_send, stream));
    return XPBD_OK;
}

// 2. wait for the peers' send events, copy every rank's row into my `recv`, record my receive event
int local_copy(xpbd_multi_world *mw, Shard &s, DeviceBuffer Shard::*send, void *recv, size_t bytes, hipStream_t stream)
{
    for (Shard &p : mw->shards) {
        if (&p != &s)
            XPBD_HIP_TRY(hipStreamWaitEvent(stream, p.ev_send, 0));
        XPBD_HIP_TRY(hipMemcpyAsync(static_cast<char *>(recv) + (size_t)p.rank * bytes, (p.*send).ptr, bytes, hipMemcpyDefault, stream));
    }
    XPBD_HIP_TRY(hipEventRecord(s.ev_recv, stream));
    return XPBD_OK;
}

// 3. wait for the peers' receive events: nobody overwrites its send buffer before every peer has read it
int local_release(xpbd_multi_world *mw, Shard &s, hipStream_t stream)
{
    for (Shard &p : mw->shards)
        if (&p != &s)
            XPBD_HIP_TRY(hipStreamWaitEvent(stream, p.ev_recv, 0));
    return XPBD_OK;
}

namespace {

// The all-gather of every local shard from this thread, on the shards' world streams (RCCL: in one group call).
int all_gather_device_raw(xpbd_multi_world *mw, size_t bytes, DeviceBuffer Shard::*send, DeviceBuffer Shard::*recv)
{
    if (mw->transport == XPBD_TRANSPORT_RCCL) {
        (void)hipGetLastError(); // see rccl_all_gather
        ncclResult_t r = mw->rccl->GroupStart();
        if (r != ncclSuccess)
            return nccl_fail(mw, r, "ncclGroupStart");
        int rc = XPBD_OK;
        for (Shard &s : mw->shards)
            if ((rc = bind(s)) != XPBD_OK || (rc = rccl_all_gather(mw, s, (s.*send).ptr, (s.*recv).ptr, bytes, s.stream)) != XPBD_OK)
                break;
        r = mw->rccl->GroupEnd(); // the group is closed whatever happened inside it
        if (rc != XPBD_OK)
            return rc;
        if (r != ncclSuccess)
            return nccl_fail(mw, r, "ncclGroupEnd");
        return XPBD_OK;
    }
    for (Shard &s : mw->shards) {
        XPBD_TRY(bind(s));
        XPBD_TRY(local_send(s, s.stream));
    }
    for (Shard &s : mw->shards) {
        XPBD_TRY(bind(s));
        XPBD_TRY(local_copy(mw, s, send, (s.*recv).ptr, bytes, s.stream));
    }
    for (Shard &s : mw->shards) {
        XPBD_TRY(bind(s));
        XPBD_TRY(local_release(mw, s, s.stream));
    }
    return XPBD_OK;
}

int all_gather_device(xpbd_multi_world *mw, size_t bytes, DeviceBuffer Shard::*send, DeviceBuffer Shard::*recv)
{
    if (int rc = all_gather_device_raw(mw, bytes, send, recv))
        return transport_broken(mw, rc);
    return XPBD_OK;
}

} // namespace

// Plan-time all-gather of host data: send[k] = `bytes` of local shard k; out = the n_ranks x bytes everybody ends up with.
// Every row is preceded by the sender's status; if any rank reports an error, every rank returns one.
int all_gather_host(xpbd_multi_world *mw, const std::vector<const void *> &send, size_t bytes, std::vector<uint8_t> &out, LocalStatus &status)
{
    const size_t row = bytes + 8;
    std::vector<uint8_t> all((size_t)mw->n_ranks * row, 0);
    const int64_t mine = status.rc;
    if (mw->shortcut()) { // every rank is here: no device round trip needed
        for (size_t k = 0; k < mw->shards.size(); ++k) {
            uint8_t *dst = all.data() + (size_t)mw->shards[k].rank * row;
            std::memcpy(dst, &mine, 8);
            if (bytes && status.ok())
                std::memcpy(dst + 8, send[k], bytes);
        }
    } else {
        std::vector<std::vector<uint8_t>> staged(mw->shards.size());
        int rc = XPBD_OK;
        auto stage = [&]() -> int {
            for (size_t k = 0; k < mw->shards.size(); ++k) {
                Shard &s = mw->shards[k];
                staged[k].assign(row, 0);
                std::memcpy(staged[k].data(), &mine, 8);
                if (bytes && status.ok())
                    std::memcpy(staged[k].data() + 8, send[k], bytes);
                XPBD_TRY(bind(s));
                XPBD_HIP_TRY(hipStreamSynchronize(s.stream)); // reserve() may free a block that is still in use
                XPBD_HIP_TRY(s.stage_send.reserve(row));
                XPBD_HIP_TRY(s.stage_recv.reserve((size_t)mw->n_ranks * row));
                XPBD_HIP_TRY(hipMemcpyAsync(s.stage_send.ptr, staged[k].data(), row, hipMemcpyHostToDevice, s.stream));
            }
            return XPBD_OK;
        };
        if ((rc = stage()) != XPBD_OK) // the staging buffers are the transport's: without them this rank cannot take part
            return transport_broken(mw, rc);
        XPBD_TRY(all_gather_device(mw, row, &Shard::stage_send, &Shard::stage_recv));
        auto collect = [&]() -> int {
            for (Shard &s : mw->shards) { // every shard takes part in the collective; the content is the same everywhere
                XPBD_TRY(bind(s));
                if (&s == &mw->shards[0])
                    XPBD_HIP_TRY(hipMemcpyAsync(all.data(), s.stage_recv.ptr, all.size(), hipMemcpyDeviceToHost, s.stream));
                XPBD_HIP_TRY(hipStreamSynchronize(s.stream));
            }
            return XPBD_OK;
        };
        if ((rc = collect()) != XPBD_OK)
            return transport_broken(mw, rc);
    }
    out.assign((size_t)mw->n_ranks * bytes, 0);
    int64_t peer_rc = 0;
    uint32_t peer = 0;
    for (uint32_t r = 0; r < mw->n_ranks; ++r) {
        int64_t st = 0;
        std::memcpy(&st, all.data() + (size_t)r * row, 8);
        if (st != 0 && peer_rc == 0) {
            peer_rc = st;
            peer = r;
        }
        if (bytes)
            std::memcpy(out.data() + (size_t)r * bytes, all.data() + (size_t)r * row + 8, bytes);
    }
    if (!status.ok())
        return status.report();
    if (peer_rc != 0)
        return set_error((int)peer_rc, "xpbd_multi_world: rank %u failed with error %d in this collective call (see its xpbd_last_error); "
                                       "every rank leaves the call with that error", peer, (int)peer_rc);
    return XPBD_OK;
}

} // namespace xpbd::multi
