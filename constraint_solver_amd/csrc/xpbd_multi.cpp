// xpbd_multi.cpp -- the multi-GPU world behind the C ABI (xpbd_multi_world_* in include/xpbd.h).
//
// EXTENSION: the reference is single-threaded and has neither body-body contacts nor any
// multi-device path; its caller is World::integrate (src/world.rs:34-43), which this replaces for an N-body world whose
// bodies are sharded over the GPUs of one node.  Parity: sharded == single device, bit for bit (tests).
//
// One xpbd_multi_world drives the LOCAL shards of a world of n_ranks shards -- all of them (a single process that owns
// every GPU of the node: what a Rust host would do) or one each (one process per GPU, the ranks of a launcher).
//
// Ownership is the LIBRARY's (xpbd_plan.hpp: slabs of space across the world's longest axis).  The first plan cuts the slabs
// (a FULL plan: every rank sees 16 bytes per body of the world); the re-plans keep the cuts, move the bodies that crossed one
// to their new owner and exchange only the RIMS of the shards (LIGHT plans: make_plan_light), until a shard is a tenth of a
// share out of balance -- then the slabs are cut anew.  The bodies themselves stay on the devices through every plan.  A
// shard is an ordinary xpbd_world in XPBD_MODE_CONTACTS holding its OWNED bodies plus GHOST copies of the remote bodies that
// can reach an owned body before the next plan, in ascending GLOBAL id (the caller's numbering) -- so every neighbour list
// and every floating-point sum has the order of the single-device run and the result is that run's, bit for bit.  Per substep:
//     narrowphase -> boundary bodies (their end-of-substep state straight into the send buffer) -> ONE all-gather (RCCL over
//     xGMI: ncclAllGather) on a communication stream, overlapping the interior bodies -> the ghosts take their owners' state
//     from the gathered buffer.
// One function enqueues a shard's frame (shard_frame), from one host thread per local shard.
// This file holds what needs a device or a communicator: the shards, the transport, the plan-time collectives around the
// planner (a handful of small all-gathers: cell keys or rims, boundary lists, the records of migrating and boundary bodies;
// no rank holds the global scene), the device half of a plan (re-pack, uploads), settings, edits, the frame, the gathers of
// reports and scene queries and the xpbd_multi_world_* ABI.  The index arithmetic lives in the host-only units: every rank's
// plan, the layout of a shard (local slots, source map, ghost rows, its joints: layout_shard) and the re-indexing of joint
// records in xpbd_plan.hpp; the merges of query hits and of the contact report with its events in xpbd_merge.hpp.
// Every plan-time all-gather carries a status word per rank and so does the frame's last one, so a rank that fails locally
// (out of memory, say) still takes part in the collectives and EVERY rank returns an error instead of the others hanging.
//
// Halo validity is checked at the END of every frame, over all ranks: if a body has used up its travel allowance since the
// plan, a remote contact may have been missed IN THAT FRAME -- the frame is undone (the state it started from is kept aside
// on the device), and either re-run after a re-plan (XPBD_MULTI_AUTO_REPLAN) or reported as XPBD_E_HALO with the state of
// the frame's start in place.  A state with possibly missed contacts never reaches the caller.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/xpbd.h"
#include "xpbd_internal.h"
#include "xpbd_merge.hpp"
#include "xpbd_plan.hpp"
#include "xpbd_rccl.h"

namespace {

using xpbd::DeviceBuffer;
using xpbd::set_error;
using namespace xpbd::plan;

constexpr uint32_t kDyn = 13;    // dynamic doubles per body: position, rotation, velocity, angular velocity
constexpr uint32_t kRigid = 38;  // sizeof(xpbd_rigid) / 8
constexpr uint32_t kRecord = 39; // a body's plan-time record: its xpbd_rigid + the shape id
struct BodyRecord {
    double v[kRecord];
};
struct Shard {
    int device = 0;
    uint32_t rank = 0;
    xpbd_world *world = nullptr;
    hipStream_t stream = nullptr;      // the shard's world stream: every kernel of the shard
    hipStream_t comm_stream = nullptr; // the per-substep halo all-gather, overlapping the interior bodies' kernels
    ncclComm_t comm = nullptr;
    hipEvent_t ev_send = nullptr, ev_recv = nullptr; // in-process transport
    hipEvent_t ev_ready = nullptr, ev_gathered = nullptr; // world stream -> communication stream -> world stream
    // The bodies this shard HOLDS (global ids, ascending): before the first plan the index slice the caller handed over,
    // after a plan the bodies it owns.  Their state lives in the shard's world on the device (slot owned_slots_h[i]) and
    // stays there through re-plans.
    std::vector<uint32_t> held_ids;
    // plan
    std::vector<uint32_t> local_ids, ghosts, boundary; // global ids (ascending): owned + ghost bodies; ghosts; mirrored owned bodies
    std::vector<uint32_t> owned_slots_h;               // local slot of held_ids[i]
    std::vector<uint8_t> far; // per owned body: more than two cells away from every foreign body (larger travel allowance)
    std::vector<uint32_t> joint_ids; // global ids (ascending) of the joints the shard's world has: local joint q = joint_ids[q]
    DeviceBuffer boundary_slots, ghost_slots, ghost_rows, owned_slots, skip_flags, disp_scale, send, recv, snapshot, disp, disp_all, stage_send, stage_recv;
    // per local slot, uploaded with the plan: the global id with XPBD_NO_HIT for the ghosts (scene queries: the OWNED bodies
    // answer, under their global ids); the global id, and 1 for the owned slots, 0 for the ghosts (contact reports)
    DeviceBuffer query_ids, report_ids, report_owned;
    double *disp_host = nullptr;   // pinned, n_ranks x {largest squared fraction of an allowance used, status}
    double *status_host = nullptr; // pinned, this process's status of the frame
    const xpbd::RcclApi *rccl = nullptr; // destroys `comm`
    xpbd::HaloLists lists() const
    {
        return xpbd::HaloLists{boundary_slots.as<uint32_t>(), (uint32_t)boundary.size(), ghost_slots.as<uint32_t>(), ghost_rows.as<uint32_t>(),
                               (uint32_t)ghosts.size(), skip_flags.as<uint8_t>(), send.as<double>(), recv.as<double>()};
    }

    ~Shard() // (then the device buffers free themselves)
    {
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        if (comm && rccl)
            (void)rccl->CommDestroy(comm);
        if (disp_host)
            (void)hipHostFree(disp_host);
        if (status_host)
            (void)hipHostFree(status_host);
        if (comm_stream)
            (void)hipStreamDestroy(comm_stream);
        for (hipEvent_t e : {ev_send, ev_ready, ev_gathered, ev_recv})
            if (e)
                (void)hipEventDestroy(e);
        xpbd_world_destroy(world);
    }
};

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

struct Workers {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    uint64_t job = 0;
    uint32_t done = 0;
    bool quit = false;
    double dt = 0.0;
    uint32_t substeps = 0;
    std::vector<ShardJob> result;
    Barrier barrier;
};

} // namespace

struct xpbd_multi_world {
    uint32_t n_ranks = 1, first_rank = 0, transport = XPBD_TRANSPORT_RCCL, flags = 0, narrowphase = XPBD_NARROWPHASE_SAT;
    double pad = 0.02, margin = 0.5;
    std::vector<Shard> shards;
    const xpbd::RcclApi *rccl = nullptr;
    bool have_shapes = false, planned = false, violated = false, broken = false;
    std::vector<double> shape_radius, shape_centroid; // per shape: max |vertex - centroid|, centroid xyz
    uint32_t n_global = 0, first_global = 0, n_bodies = 0, capacity = 1;
    std::vector<xpbd_joint> joints;
    std::vector<xpbd_joint_limit> limits; // xpbd_multi_world_set_joint_limits: GLOBAL joint indices
    std::vector<xpbd_joint_drive> drives; // xpbd_multi_world_set_joint_drives: GLOBAL joint indices
    std::vector<xpbd_collision_filter> filters; // xpbd_multi_world_set_collision_filters: [n_global] or empty (none)
    uint32_t filter_flags = 0;
    std::vector<xpbd_material> materials; // xpbd_multi_world_set_materials: [n_global] or empty (every body +inf)
    double ground_friction = std::numeric_limits<double>::infinity();
    std::vector<uint8_t> owner;        // [n_global] as of the last plan
    std::vector<uint32_t> owned_count; // [n_ranks]
    uint64_t plans = 0, rollbacks = 0, migrated = 0, steps = 0, ns_enqueue = 0, ns_wait_broadphase = 0, ns_wait_frame = 0, ns_plan = 0;
    double cell_edge = 0.0;
    double rmax_local = 0.0;          // largest bounding radius (r_shape + |centroid - com|) among the bodies this process handed over
    std::vector<int32_t> slot_of;     // [n_global] scratch of a plan: local slot of a body, -1 outside the shard being built
    JointLists joint_lists;           // the joints at every body (indices into `joints`, ascending)
    std::vector<Cut> cuts;            // the cuts of the last full plan, kept by the light plans between (cuts_valid)
    int cut_axes[3] = {0, 1, 2};      // ... over slab keys packed in this order of the axes
    bool cuts_valid = false, check_plans = false, plan_torn = false;
    uint32_t balance_most = 0, balance_least = 0; // most / fewest bodies of a rank right after the last full plan
    uint64_t full_plans = 0, light_plans = 0;
    double last_displacement = 0.0; // the largest fraction of its travel allowance any body had used at the last check, times halo_margin
    Workers *workers = nullptr;     // one enqueueing thread per local shard (n_local > 1), started by the first step
    // contact reports (xpbd_multi_world_set_contact_report): the whole world's report of the last frame, gathered on every rank
    // when the frame has been accepted (before a re-plan repacks the shards), and the touching pairs of the frame before it
    bool report_on = false, report_valid = false;
    std::vector<xpbd_pair_contact> report_pairs;
    std::vector<xpbd_contact_point> report_points;
    std::vector<xpbd_contact_event> report_events;
    std::vector<uint64_t> report_prev; // keys (a << 32 | b) of the previous frame's touching pairs; empty: S_prev is empty
    uint32_t report_begins = 0;
    ~xpbd_multi_world(); // stops the workers (then the shards go)
    bool all_local() const { return shards.size() == n_ranks; }
    bool shortcut() const { return all_local() && !(flags & XPBD_MULTI_PLAN_THROUGH_DEVICE); } // plan-time gathers are memcpys
    uint32_t rows_per_rank() const { return capacity; }
    Shard *local_shard(uint32_t rank) { return rank >= first_rank && rank < first_rank + shards.size() ? &shards[rank - first_rank] : nullptr; }
};

namespace {

uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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

// Closes the function-try-block of every xpbd_multi_world_* call (but create): an exception leaves the shards in an unknown
// state and maybe the peers inside a collective, so it breaks the transport (see XPBD_ABI_CATCH).
#define XPBD_MULTI_ABI_CATCH \
    catch (...) { return transport_broken(mw, xpbd::abi_exception(__func__)); }

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

// Variable-length lists of T from every rank: `local` holds every local shard's list; gather_counts (one collective for the
// lengths of all the lists it is given) yields `counts` and `widest`, gather_rows (one collective) pads every local list to
// `widest` (value-initialised entries: no reader looks past counts[r]) and yields `rows`.  Both carry `st` as all_gather_host
// does: a failed shard takes part with whatever it holds.
template <class T> struct RankLists {
    std::vector<std::vector<T>> local;
    std::vector<uint32_t> counts; // per rank
    uint32_t widest = 1;          // the longest list, at least 1
    std::vector<uint8_t> rows;    // n_ranks x widest x T
    explicit RankLists(size_t n_local) : local(n_local) {}
    T at(uint32_t rank, uint32_t i) const
    {
        T v;
        std::memcpy(&v, rows.data() + ((size_t)rank * widest + i) * sizeof v, sizeof v);
        return v;
    }
};

template <class... T> int gather_counts(xpbd_multi_world *mw, LocalStatus &st, RankLists<T> &...lists)
{
    constexpr size_t N = sizeof...(T);
    const size_t nl = mw->shards.size();
    std::vector<std::array<uint32_t, N>> mine(nl);
    std::vector<const void *> send(nl);
    for (size_t k = 0; k < nl; ++k) {
        mine[k] = {(uint32_t)lists.local[k].size()...};
        send[k] = mine[k].data();
    }
    std::vector<uint8_t> gathered;
    XPBD_TRY(all_gather_host(mw, send, N * sizeof(uint32_t), gathered, st));
    size_t column = 0;
    auto take = [&](std::vector<uint32_t> &counts, uint32_t &widest) {
        counts.resize(mw->n_ranks);
        for (uint32_t r = 0; r < mw->n_ranks; ++r) {
            std::memcpy(&counts[r], gathered.data() + ((size_t)r * N + column) * sizeof(uint32_t), sizeof(uint32_t));
            widest = std::max(widest, counts[r]);
        }
        ++column;
    };
    (take(lists.counts, lists.widest), ...);
    return XPBD_OK;
}

template <class T> int gather_rows(xpbd_multi_world *mw, LocalStatus &st, RankLists<T> &list)
{
    std::vector<const void *> send;
    for (std::vector<T> &l : list.local) {
        l.resize(list.widest);
        send.push_back(l.data());
    }
    return all_gather_host(mw, send, (size_t)list.widest * sizeof(T), list.rows, st);
}

template <class T>
int upload_vector(DeviceBuffer &buf, const std::vector<T> &v, hipStream_t stream)
{
    XPBD_HIP_TRY(buf.reserve(std::max<size_t>(v.size() * sizeof(T), 8)));
    if (!v.empty())
        XPBD_HIP_TRY(hipMemcpyAsync(buf.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return XPBD_OK;
}

struct KeyRow {
    int64_t key;
    uint32_t id, unused;
};

// XPBD_MULTI_TRACE_PLAN=1: the host time of every phase of a plan on stderr
struct PlanTrace {
    uint64_t plan = 0, t_last = 0;
    bool on = false;
    explicit PlanTrace(uint64_t plan_index) : plan(plan_index), t_last(now_ns())
    {
        static const bool trace = std::getenv("XPBD_MULTI_TRACE_PLAN") != nullptr;
        on = trace;
    }
    void lap(const char *what)
    {
        if (on) {
            const uint64_t t = now_ns();
            std::fprintf(stderr, "[xpbd plan %llu] %-28s %8.3f ms\n", (unsigned long long)plan, what, (double)(t - t_last) * 1e-6);
            t_last = t;
        }
    }
};

// The cell keys of the bodies every local shard holds, computed where the bodies are (8 bytes per body come back).
int held_cell_keys(xpbd_multi_world *mw, LocalStatus &st, double edge, std::vector<std::vector<int64_t>> &held_keys)
{
    held_keys.assign(mw->shards.size(), std::vector<int64_t>());
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        Shard &s = mw->shards[k];
        const uint32_t cnt = (uint32_t)s.held_ids.size();
        held_keys[k].assign(cnt, 0);
        uint32_t bad = UINT32_MAX;
        if (st.ok())
            st.keep(xpbd::halo_cell_keys(s.world, s.owned_slots.as<uint32_t>(), cnt, edge, held_keys[k].data(), &bad));
        if (st.ok() && bad != UINT32_MAX)
            st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u has a non-finite position: it cannot be placed in the grid the shards "
                                              "are cut from", s.held_ids[bad]));
    }
    return XPBD_OK;
}

// One all-gather of 16 bytes per body: the cell key of every body of the world and who holds it.
int gather_world_keys(xpbd_multi_world *mw, LocalStatus &st, const std::vector<std::vector<int64_t>> &held_keys, uint64_t max_held,
                      std::vector<int64_t> &keys, std::vector<uint8_t> &holder)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    std::vector<std::vector<KeyRow>> key_rows(n_local);
    std::vector<const void *> send(n_local);
    std::vector<uint8_t> gathered;
    for (size_t k = 0; k < n_local; ++k) {
        const Shard &s = mw->shards[k];
        key_rows[k].assign(max_held, KeyRow{0, UINT32_MAX, 0});
        for (size_t i = 0; i < s.held_ids.size() && st.ok(); ++i)
            key_rows[k][i] = KeyRow{held_keys[k][i], s.held_ids[i], 0};
        send[k] = key_rows[k].data();
    }
    XPBD_TRY(all_gather_host(mw, send, (size_t)max_held * sizeof(KeyRow), gathered, st));
    keys.assign(n, 0);
    holder.assign(n, 0xFF);
    for (uint32_t r = 0; r < w && st.ok(); ++r) {
        const KeyRow *rows = reinterpret_cast<const KeyRow *>(gathered.data() + (size_t)r * max_held * sizeof(KeyRow));
        for (uint64_t i = 0; i < max_held; ++i) {
            if (rows[i].id == UINT32_MAX)
                break;
            if (rows[i].id >= n || holder[rows[i].id] != 0xFF) {
                st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u is held twice or out of range (rank %u)", rows[i].id, r));
                break;
            }
            keys[rows[i].id] = rows[i].key;
            holder[rows[i].id] = (uint8_t)r;
        }
    }
    return XPBD_OK;
}

// ---- body-indexed settings: the world's copy (global indices) handed to a shard (local slots) -------------------------------
// Called for every shard after every plan (a body takes its settings along when it changes owner) and by the setters.
// local_ids: global id of every local slot, owned bodies and ghosts alike -- an owned-ghost pair is decided on this shard, and a
// ghost's coefficient enters the min of an owned-ghost contact.
using PushSetting = int (*)(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids);

// The rows of a per-body table of the world at the local slots; an empty table (the default) stays empty.
template <class T> std::vector<T> local_rows(const std::vector<T> &global, const std::vector<uint32_t> &local_ids)
{
    std::vector<T> local(global.empty() ? 0 : local_ids.size());
    for (size_t q = 0; q < local.size(); ++q)
        local[q] = global[local_ids[q]];
    return local;
}

// The records (limits or drives) on the joints of shard s, in the shard's joint numbering (local_joint_records), handed to the
// shard's setter.
template <class Record> int push_joint_records(const std::vector<Record> &global, const Shard &s, int (*set)(xpbd_world *, const Record *, uint32_t))
{
    const std::vector<Record> local = local_joint_records(global, s.joint_ids);
    return set(s.world, local.data(), (uint32_t)local.size());
}

int push_joint_limits(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &) { return push_joint_records(mw->limits, s, xpbd_world_set_joint_limits); }

int push_joint_drives(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &) { return push_joint_records(mw->drives, s, xpbd_world_set_joint_drives); }

int push_collision_filters(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    const std::vector<xpbd_collision_filter> local = local_rows(mw->filters, local_ids);
    return xpbd_world_set_collision_filters(s.world, local.empty() ? nullptr : local.data(), (uint32_t)local.size(), mw->filter_flags);
}

int push_materials(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    const std::vector<xpbd_material> local = local_rows(mw->materials, local_ids);
    return xpbd_world_set_materials(s.world, local.empty() ? nullptr : local.data(), (uint32_t)local.size(), mw->ground_friction);
}

// Every body-indexed setting of the world on shard s (its joints are set: the limits name them).  A new setting is added here.
int push_body_settings(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    for (PushSetting push : {push_joint_limits, push_joint_drives, push_collision_filters, push_materials})
        XPBD_TRY(push(mw, s, local_ids));
    return XPBD_OK;
}

// The tail of a setter: the checked and recorded setting goes to every shard of a planned world (the plan hands it over
// otherwise).  Only a device failure fails here, and the shards disagree then.
int push_to_shards(xpbd_multi_world *mw, PushSetting push, const char *what)
{
    if (!mw->planned)
        return XPBD_OK;
    for (Shard &s : mw->shards) {
        int rc = bind(s);
        if (rc == XPBD_OK)
            rc = push(mw, s, s.local_ids);
        if (rc != XPBD_OK) {
            mw->broken = true;
            return set_error(rc, "%s -- the shards' %s disagree now: destroy this xpbd_multi_world", xpbd_last_error(), what);
        }
    }
    return XPBD_OK;
}

// Body edits (include/xpbd.h, "Body EDITS") reach every local shard that HOLDS the body, as owner or as ghost (slot_in_shard
// over the shard's local_ids).
// The tail of an edit: a shard that fails here has not done what the others did.
int edit_failed(xpbd_multi_world *mw, int rc, const char *what)
{
    mw->broken = true;
    return set_error(rc, "%s -- the shards' %s disagree now: destroy this xpbd_multi_world", xpbd_last_error(), what);
}

// The second half of every plan: the boundary lists of all ranks fix the rows of the per-substep all-gather, the records of
// the bodies that change hands or are mirrored travel, and every shard's local world is re-packed on its device.  Collective.
int finish_plan(xpbd_multi_world *mw, LocalStatus &st, std::vector<ShardPlan> &plans, double edge, PlanTrace &trace)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    // 4. the boundary lists of all ranks (ascending global ids) fix the rows of the per-substep all-gather; the export lists
    //    those of the plan-time record exchange
    RankLists<uint32_t> boundary(n_local), exports(n_local);
    RankLists<BodyRecord> records(n_local);
    for (size_t k = 0; k < n_local && st.ok(); ++k)
        boundary.local[k] = plans[k].boundary, exports.local[k] = plans[k].exports;
    XPBD_TRY(gather_counts(mw, st, boundary, exports));
    XPBD_TRY(gather_rows(mw, st, boundary));
    // the records of the exported bodies: gathered on the device that holds them, 39 doubles each (nothing to exchange if
    // nobody exports anything: every rank sees that in the gathered counts)
    if (std::any_of(exports.counts.begin(), exports.counts.end(), [](uint32_t c) { return c > 0; })) {
        XPBD_TRY(gather_rows(mw, st, exports));
        records.counts = exports.counts, records.widest = exports.widest;
        std::vector<uint32_t> slots;
        for (size_t k = 0; k < n_local; ++k) {
            Shard &s = mw->shards[k];
            records.local[k].resize(records.widest);
            slots.clear();
            if (st.ok())
                for (uint32_t g : plans[k].exports)
                    slots.push_back(s.owned_slots_h[std::lower_bound(s.held_ids.begin(), s.held_ids.end(), g) - s.held_ids.begin()]);
            if (st.ok())
                st.keep(xpbd::download_records(s.world, slots.data(), (uint32_t)slots.size(), records.local[k][0].v));
        }
        XPBD_TRY(gather_rows(mw, st, records));
    }
    trace.lap("lists, exported records");

    // 5. every shard's local world: owned + ghost bodies in ascending global id (layout_shard), re-packed on its device
    const uint32_t rows = boundary.widest; // (rows per rank of the per-substep all-gather from now on: mw->capacity, set when the plan has succeeded)
    const RankIds boundary_ids{reinterpret_cast<const uint32_t *>(boundary.rows.data()), boundary.counts.data(), boundary.widest, w};
    const RankIds export_ids{reinterpret_cast<const uint32_t *>(exports.rows.data()), exports.counts.data(), exports.widest, w};
    const JointIndex ji = mw->joint_lists.view(mw->joints.data());
    if (mw->slot_of.size() != n)
        mw->slot_of.assign(n, -1);
    auto build_shard = [&](size_t k) -> int {
        Shard &s = mw->shards[k];
        ShardPlan &pl = plans[k];
        XPBD_TRY(bind(s));
        ShardLayout lay;
        XPBD_TRY(layout_shard(s.rank, pl, s.held_ids, s.owned_slots_h, boundary_ids, export_ids, rows, ji, mw->slot_of, mw->margin, edge, lay));
        std::vector<BodyRecord> incoming(lay.incoming.size());
        for (size_t i = 0; i < incoming.size(); ++i)
            incoming[i] = records.at(lay.incoming[i].holder, lay.incoming[i].row);
        const uint32_t n_own = (uint32_t)pl.own.size(), n_loc = (uint32_t)lay.local_ids.size();
        trace.lap("  source map of a shard");
        if (int rc = xpbd::repack_bodies(s.world, lay.src.data(), n_loc, incoming.empty() ? nullptr : incoming[0].v, (uint32_t)incoming.size()))
            return rc;
        trace.lap("  re-pack on the device");
        if (int rc = xpbd_world_set_joints(s.world, lay.joints.data(), (uint32_t)lay.joints.size()))
            return rc;
        s.joint_ids.swap(lay.joint_ids);
        XPBD_TRY(push_body_settings(mw, s, lay.local_ids));
        XPBD_HIP_TRY(hipStreamSynchronize(s.stream));
        trace.lap("  joints");
        XPBD_TRY(upload_vector(s.boundary_slots, lay.boundary_slots, s.stream));
        XPBD_TRY(upload_vector(s.ghost_slots, lay.ghost_slots, s.stream));
        XPBD_TRY(upload_vector(s.ghost_rows, lay.ghost_rows, s.stream));
        XPBD_TRY(upload_vector(s.owned_slots, lay.owned_slots, s.stream));
        XPBD_TRY(upload_vector(s.skip_flags, lay.skip, s.stream));
        XPBD_TRY(upload_vector(s.disp_scale, lay.disp_scale, s.stream));
        XPBD_TRY(upload_vector(s.query_ids, lay.query_ids, s.stream));
        XPBD_TRY(upload_vector(s.report_ids, lay.local_ids, s.stream));
        XPBD_TRY(upload_vector(s.report_owned, lay.owned, s.stream));
        XPBD_HIP_TRY(s.send.reserve((size_t)rows * kDyn * 8));
        XPBD_HIP_TRY(s.recv.reserve((size_t)w * rows * kDyn * 8));
        XPBD_HIP_TRY(hipMemsetAsync(s.send.ptr, 0, (size_t)rows * kDyn * 8, s.stream));
        XPBD_HIP_TRY(s.snapshot.reserve(std::max<size_t>((size_t)3 * n_own * 8, 8)));
        XPBD_HIP_TRY(s.disp.reserve(16));
        XPBD_HIP_TRY(s.disp_all.reserve((size_t)w * 16));
        if (int rc = xpbd_world_snapshot_positions(s.world, s.owned_slots.as<uint32_t>(), n_own, s.snapshot.as<double>()))
            return rc;
        XPBD_HIP_TRY(hipStreamSynchronize(s.stream)); // the layout's host vectors go out of scope
        s.owned_slots_h.swap(lay.owned_slots);
        s.local_ids.swap(lay.local_ids);
        s.held_ids.swap(pl.own); // from now on the shard holds what it owns
        s.ghosts.swap(pl.ghosts);
        s.boundary.swap(pl.boundary);
        s.far.swap(pl.far);
        trace.lap("  index lists of a shard");
        return XPBD_OK;
    };
    for (size_t k = 0; k < n_local && st.ok(); ++k) {
        st.keep(build_shard(k));
        if (!st.ok())
            mw->plan_torn = true; // some shards re-packed, this one half-way: there is no plan to go back to (see make_plan)
    }
    // all ranks leave the plan together: a last status-only exchange (a failed re-pack on one rank fails the plan everywhere)
    std::vector<uint8_t> gathered;
    if (int rc = all_gather_host(mw, std::vector<const void *>(n_local, nullptr), 0, gathered, st)) {
        mw->plan_torn = true; // (a shard of some rank failed while being re-packed)
        return rc;
    }
    mw->capacity = rows;
    mw->cell_edge = edge;
    mw->planned = true;
    mw->violated = false;
    mw->last_displacement = 0.0;
    ++mw->plans;
    return XPBD_OK;
}

double plan_cell_edge(const xpbd_multi_world *mw, double rmax) { return 2.0 * (rmax + mw->pad + mw->margin); }

// (rmax of the world, bodies held per rank): the first collective of every plan
int gather_heads(xpbd_multi_world *mw, LocalStatus &st, double &rmax, uint64_t &max_held)
{
    struct Head {
        double rmax;
        uint64_t count;
    };
    const size_t n_local = mw->shards.size();
    std::vector<Head> head(n_local);
    std::vector<const void *> send(n_local);
    std::vector<uint8_t> gathered;
    for (size_t k = 0; k < n_local; ++k) {
        head[k] = Head{mw->rmax_local, mw->shards[k].held_ids.size()};
        send[k] = &head[k];
    }
    XPBD_TRY(all_gather_host(mw, send, sizeof(Head), gathered, st));
    rmax = 0.0, max_held = 0;
    uint64_t total_held = 0;
    for (uint32_t r = 0; r < mw->n_ranks; ++r) {
        Head h;
        std::memcpy(&h, gathered.data() + (size_t)r * sizeof(Head), sizeof h);
        rmax = std::max(rmax, h.rmax);
        max_held = std::max(max_held, h.count);
        total_held += h.count;
    }
    const double edge = plan_cell_edge(mw, rmax);
    if (!(edge > 0.0) || !(edge <= 1.0e300))
        st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: cell edge %g from radius %g, pad %g, halo_margin %g", edge, rmax, mw->pad, mw->margin));
    if (total_held != mw->n_global)
        st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: the ranks hold %llu bodies together, the world has %u", (unsigned long long)total_held,
                          mw->n_global));
    return XPBD_OK;
}

// A FULL plan: ownership re-cut from the cell keys of the whole world (every rank passes over 16 bytes per body of it), halos
// from the global keys and owners.  The first plan, and whenever the sticky cuts of the light plans have drifted out of balance.
// The bodies stay on the device: what crosses the bus is 8 bytes of cell key per owned body, the records of the bodies that
// change hands or are mirrored (a few per cent) and the index lists of the new plan.  Collective.  Local failures are
// carried through the collectives (LocalStatus: `st` may already hold one), so all ranks fail together.
int make_plan_full(xpbd_multi_world *mw, LocalStatus &st, PlanTrace &trace)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    // 1. the largest bounding radius of the whole world (r_shape + |centroid - com|: conservative whatever the rotation;
    //    a property of the bodies, known since the upload) and how many bodies every rank owns
    double rmax = 0.0;
    uint64_t max_held = 0;
    XPBD_TRY(gather_heads(mw, st, rmax, max_held));
    const double edge = plan_cell_edge(mw, rmax);
    // 2. grid cell of every body of the world (centre = position + center_of_mass)
    std::vector<std::vector<int64_t>> held_keys;
    XPBD_TRY(held_cell_keys(mw, st, edge, held_keys));
    trace.lap("cell keys (device)");
    std::vector<int64_t> keys;
    std::vector<uint8_t> holder;
    XPBD_TRY(gather_world_keys(mw, st, held_keys, max_held, keys, holder));
    trace.lap("keys of the world");

    // 3. ownership: the cell sequence (longest axis first) cut into runs of near-equal body count; then who mirrors whom
    std::vector<uint8_t> owner(n, 0);
    std::vector<uint32_t> owned_count(w, 0);
    std::vector<ShardPlan> plans(n_local);
    uint64_t migrated = 0;
    if (st.ok()) {
        compute_owners(keys.data(), n, w, owner.data(), mw->cuts, mw->cut_axes);
        for (uint32_t g = 0; g < n; ++g) {
            ++owned_count[owner[g]];
            migrated += owner[g] != holder[g];
        }
        trace.lap("cuts, owners");
        for (size_t k = 0; k < n_local; ++k)
            full_rank_plan(mw->shards[k].rank, mw->shards[k].held_ids, keys.data(), owner.data(), holder.data(), n, mw->joints.data(),
                           (uint32_t)mw->joints.size(), plans[k]);
    }
    trace.lap("halo plans");
    XPBD_TRY(finish_plan(mw, st, plans, edge, trace));
    mw->owner.swap(owner);
    mw->owned_count.swap(owned_count);
    mw->migrated = migrated;
    mw->cuts_valid = true;
    mw->balance_most = 0, mw->balance_least = UINT32_MAX;
    for (uint32_t c : mw->owned_count) {
        mw->balance_most = std::max(mw->balance_most, c);
        mw->balance_least = std::min(mw->balance_least, c);
    }
    ++mw->full_plans;
    return XPBD_OK;
}

// A LIGHT plan: the cuts stay where the last full plan put them, so a body's owner follows from its own cell key, and what a
// rank must know of the others is the RIM -- the bodies within two layers of a cut (nobody else can lie within two cells of a
// foreign cell), the bodies that change owner, and the ends of joints that leave their holder.  Host work and traffic are
// proportional to the rank's own bodies plus the rims, not to the world.  Falls back to a full plan (same collectives on
// every rank: the decision is taken from gathered data) when the shards have drifted out of balance.
int make_plan_light(xpbd_multi_world *mw, LocalStatus &st, PlanTrace &trace, bool &done)
{
    done = false;
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    std::vector<uint8_t> gathered;
    std::vector<const void *> send(n_local);
    double rmax = 0.0;
    uint64_t max_held = 0;
    XPBD_TRY(gather_heads(mw, st, rmax, max_held));
    const double edge = plan_cell_edge(mw, rmax);
    std::vector<std::vector<int64_t>> held_keys;
    XPBD_TRY(held_cell_keys(mw, st, edge, held_keys));
    trace.lap("cell keys (device)");
    // the new owner of every held body from the sticky cuts; how many bodies every rank sends to every rank
    std::vector<std::vector<uint8_t>> held_owner(n_local);
    std::vector<std::vector<int64_t>> held_slab(n_local);
    std::vector<std::vector<uint32_t>> tally(n_local, std::vector<uint32_t>(w, 0));
    for (size_t k = 0; k < n_local; ++k) {
        const Shard &s = mw->shards[k];
        held_owner[k].assign(s.held_ids.size(), (uint8_t)s.rank);
        held_slab[k].assign(s.held_ids.size(), 0);
        for (size_t i = 0; i < s.held_ids.size() && st.ok(); ++i) {
            held_slab[k][i] = slab_key(held_keys[k][i], mw->cut_axes);
            held_owner[k][i] = (uint8_t)owner_of(mw->cuts, held_slab[k][i], s.held_ids[i]);
            ++tally[k][held_owner[k][i]];
        }
        send[k] = tally[k].data();
    }
    XPBD_TRY(all_gather_host(mw, send, (size_t)w * 4, gathered, st));
    std::vector<uint32_t> owned_count(w, 0);
    uint64_t migrated = 0;
    for (uint32_t h = 0; h < w; ++h)
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t c;
            std::memcpy(&c, gathered.data() + ((size_t)h * w + r) * 4, 4);
            owned_count[r] += c;
            if (h != r)
                migrated += c;
        }
    {
        // out of balance (a tenth of a share off): time for new cuts
        const uint32_t share = std::max(1u, n / w);
        uint32_t most = 0, least = UINT32_MAX;
        for (uint32_t c : owned_count) {
            most = std::max(most, c);
            least = std::min(least, c);
        }
        // (against what the last full plan achieved: cuts snap to cell boundaries, a world of few cells is never even)
        if (most > mw->balance_most + share / 10 + 8 || least + share / 10 + 8 < mw->balance_least)
            return XPBD_OK; // (done stays false: the caller makes a full plan; every rank decides alike)
    }
    trace.lap("owners from the cuts");
    // the rims: (key, id, new owner) of the held bodies near a cut, changing owner, or at the end of a joint that leaves the shard
    const std::vector<int64_t> cut_layers = cut_layers_of(mw->cuts);
    const JointIndex ji = mw->joint_lists.view(mw->joints.data());
    RankLists<RimRow> rim(n_local);
    if (mw->slot_of.size() != n)
        mw->slot_of.assign(n, -1);
    for (size_t k = 0; k < n_local && st.ok(); ++k)
        rim_rows_of(mw->shards[k].rank, mw->shards[k].held_ids, held_keys[k], held_owner[k], held_slab[k], cut_layers, ji, mw->slot_of, rim.local[k]);
    XPBD_TRY(gather_counts(mw, st, rim));
    XPBD_TRY(gather_rows(mw, st, rim));
    if (trace.on)
        std::fprintf(stderr, "[xpbd plan %llu] rim rows per rank: up to %u\n", (unsigned long long)mw->plans, rim.widest);
    trace.lap("rims of the world");
    // everybody's rim by body id: (key, owner, holder)
    KnownMap known;
    if (st.ok()) {
        size_t total = 0;
        for (uint32_t c : rim.counts)
            total += c;
        known.reserve(total * 2 + 16);
        for (uint32_t h = 0; h < w && st.ok(); ++h) {
            for (uint32_t i = 0; i < rim.counts[h]; ++i) {
                const RimRow row = rim.at(h, i);
                if (row.id >= n || row.owner >= w || !known.emplace(row.id, Known{row.key, row.owner, (uint8_t)h}).second) {
                    st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u is held twice or out of range (rank %u)", row.id, h));
                    break;
                }
            }
        }
    }
    std::vector<ShardPlan> plans(n_local);
    for (size_t k = 0; k < n_local && st.ok(); ++k) {
        Shard &s = mw->shards[k];
        ShardPlan &pl = plans[k];
        st.keep(light_rank_plan(s.rank, s.held_ids, held_keys[k], held_owner[k], known, ji, mw->slot_of, pl));
        if (!st.ok())
            break;
        if (pl.own.size() != owned_count[s.rank]) {
            st.keep(set_error(XPBD_E_HIP, "xpbd_multi_world: rank %u is to own %u bodies but finds %zu (inconsistent plans)", s.rank, owned_count[s.rank],
                              pl.own.size()));
            break;
        }
        exports_of(s.rank, s.held_ids, held_owner[k], pl.boundary, pl.exports);
    }
    trace.lap("halo plans (light)");
    if (mw->check_plans) { // XPBD_MULTI_CHECK_PLANS=1: the same lists from the keys of the whole world (the full planner, same cuts)
        std::vector<int64_t> keys;
        std::vector<uint8_t> holder;
        XPBD_TRY(gather_world_keys(mw, st, held_keys, max_held, keys, holder));
        if (st.ok()) {
            std::vector<uint8_t> owner(n);
            for (uint32_t g = 0; g < n; ++g)
                owner[g] = (uint8_t)owner_of(mw->cuts, slab_key(keys[g], mw->cut_axes), g);
            for (size_t k = 0; k < n_local && st.ok(); ++k) {
                std::vector<uint32_t> own, ghosts, boundary;
                std::vector<uint8_t> far;
                HaloPlanner::plan_rank(keys.data(), owner.data(), n, mw->shards[k].rank, mw->joints.data(), (uint32_t)mw->joints.size(), own, ghosts, boundary, &far);
                const ShardPlan &pl = plans[k];
                if (own != pl.own || ghosts != pl.ghosts || boundary != pl.boundary || far != pl.far)
                    st.keep(set_error(XPBD_E_HIP, "xpbd_multi_world: the light plan of rank %u differs from the full planner's (own %zu / %zu, ghosts %zu / %zu, "
                                                  "boundary %zu / %zu)", mw->shards[k].rank, pl.own.size(), own.size(), pl.ghosts.size(), ghosts.size(),
                                      pl.boundary.size(), boundary.size()));
            }
        }
        trace.lap("checked against the full planner");
    }
    XPBD_TRY(finish_plan(mw, st, plans, edge, trace));
    mw->owner.clear(); // (rebuilt on demand: xpbd_multi_world_owners)
    mw->owned_count.swap(owned_count);
    mw->migrated = migrated;
    ++mw->light_plans;
    done = true;
    return XPBD_OK;
}

// Builds ownership and halos from the bodies the shards own AT THE MOMENT (the first time: the index slices the caller handed
// over, uploaded as they are) and re-packs every shard's local world.  Collective.
int make_plan(xpbd_multi_world *mw, LocalStatus &st)
{
    const uint64_t t_plan = now_ns();
    PlanTrace trace(mw->plans);
    bool done = false;
    int rc = XPBD_OK;
    if (mw->cuts_valid && mw->n_ranks > 1 && !(mw->flags & XPBD_MULTI_FULL_PLANS))
        rc = make_plan_light(mw, st, trace, done);
    if (rc == XPBD_OK && !done)
        rc = make_plan_full(mw, st, trace);
    mw->ns_plan += now_ns() - t_plan;
    if (rc != XPBD_OK && mw->plan_torn && !mw->broken) {
        // A plan that fails BEFORE any shard is re-packed leaves the old plan and the state as they were (every rank returns
        // the error); one that fails in the middle of the re-packing does not: the world cannot be used any more.
        mw->broken = true;
        return set_error(rc, "%s -- the shards were being re-packed: destroy this xpbd_multi_world on every rank", xpbd_last_error());
    }
    return rc;
}

// The owned bodies' current state (ascending global id, like Shard::held_ids), for a download.
int fetch_owned(xpbd_multi_world *mw, std::vector<std::vector<double>> &held)
{
    held.assign(mw->shards.size(), std::vector<double>());
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        Shard &s = mw->shards[k];
        XPBD_TRY(bind(s));
        const uint32_t n_loc = (uint32_t)s.local_ids.size();
        std::vector<double> aos((size_t)n_loc * kRigid);
        if (int rc = xpbd_world_download_bodies(s.world, reinterpret_cast<xpbd_rigid *>(aos.data()), n_loc))
            return rc;
        held[k].resize(s.held_ids.size() * kRigid);
        for (size_t i = 0; i < s.held_ids.size(); ++i)
            std::memcpy(&held[k][i * kRigid], &aos[(size_t)s.owned_slots_h[i] * kRigid], kRigid * 8);
    }
    return XPBD_OK;
}

int replan(xpbd_multi_world *mw)
{
    LocalStatus st;
    return make_plan(mw, st);
}

// One frame of local shard k and, behind it, the end-of-frame exchange: per rank the largest fraction of its travel allowance
// any owned body has used since the plan (squared) and the rank's status.  Enqueued by one thread per shard: the caller's
// with one local shard, worker k's with several (enqueue_frame).  The collectives, per thread:
//   RCCL   ncclAllGather on the shard's own communicator (one thread per device, no group call);
//   local  local_send | BARRIER | local_copy | BARRIER | local_release.
// A local error (job.st) skips the shard's remaining launches, the collectives still run; a collective that could not be
// enqueued (job.fatal) skips the shard's remaining collectives.  Every thread passes every barrier whatever went wrong, so
// nobody is left waiting.
void shard_frame(xpbd_multi_world *mw, size_t k, double dt, uint32_t substeps, ShardJob &job, Barrier &bar) noexcept
{
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
    const size_t bytes = (size_t)mw->rows_per_rank() * kDyn * 8;
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

void worker_main(xpbd_multi_world *mw, size_t k)
{
    Workers &w = *mw->workers;
    uint64_t seen = 0;
    for (;;) {
        double dt;
        uint32_t substeps;
        {
            std::unique_lock<std::mutex> lock(w.m);
            w.cv_job.wait(lock, [&] { return w.quit || w.job != seen; });
            if (w.quit)
                return;
            seen = w.job;
            dt = w.dt, substeps = w.substeps;
        }
        w.result[k] = ShardJob();
        shard_frame(mw, k, dt, substeps, w.result[k], w.barrier);
        {
            std::lock_guard<std::mutex> lock(w.m);
            ++w.done;
        }
        w.cv_done.notify_one();
    }
}

void stop_workers(xpbd_multi_world *mw) noexcept;

// Runs shard_frame on every worker (started by the first call) and waits until all of them have enqueued their frames.
// Workers that cannot all be started are stopped again (mw->workers stays NULL) and the exception goes on to the caller's
// handler, which breaks the world like any host failure of a step: remote ranks may already wait in this frame's collectives.
int run_workers(xpbd_multi_world *mw, double dt, uint32_t substeps)
{
    if (!mw->workers) {
        mw->workers = new Workers;
        try {
            Workers &w = *mw->workers;
            w.result.resize(mw->shards.size());
            w.barrier.n = (uint32_t)mw->shards.size();
            for (size_t k = 0; k < mw->shards.size(); ++k)
                w.threads.emplace_back(worker_main, mw, k);
        } catch (...) {
            stop_workers(mw);
            throw;
        }
    }
    Workers &w = *mw->workers;
    std::unique_lock<std::mutex> lock(w.m);
    w.dt = dt, w.substeps = substeps, w.done = 0;
    ++w.job;
    w.cv_job.notify_all();
    w.cv_done.wait(lock, [&] { return w.done == (uint32_t)w.threads.size(); });
    return XPBD_OK;
}

// Enqueues one whole frame on every local shard (shard_frame): on this thread with one local shard, on the workers with
// several.  Local errors are kept in `st` (the first in shard order); a collective that could not be enqueued breaks the
// transport.
int enqueue_frame(xpbd_multi_world *mw, double dt, uint32_t substeps, LocalStatus &st)
{
    const uint64_t t0 = now_ns();
    ShardJob alone;
    const ShardJob *jobs = &alone;
    if (mw->shards.size() == 1) {
        Barrier bar; // one party: arrive_and_wait passes straight through
        shard_frame(mw, 0, dt, substeps, alone, bar);
    } else {
        XPBD_TRY(run_workers(mw, dt, substeps));
        jobs = mw->workers->result.data();
    }
    uint64_t wait = 0;
    for (size_t k = 0; k < mw->shards.size(); ++k)
        wait = std::max(wait, jobs[k].ns_wait_broadphase);
    mw->ns_wait_broadphase += wait;
    mw->ns_enqueue += (now_ns() - t0) - wait;
    for (size_t k = 0; k < mw->shards.size(); ++k)
        if (!jobs[k].fatal.ok())
            return transport_broken(mw, jobs[k].fatal.report());
    for (size_t k = 0; k < mw->shards.size() && st.ok(); ++k)
        st = jobs[k].st;
    return XPBD_OK;
}

void stop_workers(xpbd_multi_world *mw) noexcept
{
    if (!mw->workers)
        return;
    {
        std::lock_guard<std::mutex> lock(mw->workers->m);
        mw->workers->quit = true;
    }
    mw->workers->cv_job.notify_all();
    for (std::thread &t : mw->workers->threads)
        t.join();
    delete mw->workers;
    mw->workers = nullptr;
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
    mw->ns_wait_frame += now_ns() - t0;
    *moved = std::sqrt(worst) * mw->margin; // "margin-equivalent" metres: halo_margin means the allowance is used up
    if (!st.ok())
        return st.report();
    if (peer_rc != 0)
        return set_error((int)peer_rc, "xpbd_multi_world_step: rank %u failed with error %d in this frame (see its xpbd_last_error); the frame "
                                       "is undone on every rank", peer, (int)peer_rc);
    return XPBD_OK;
}

} // namespace

xpbd_multi_world::~xpbd_multi_world() { stop_workers(this); }

namespace {

int restore_frame(xpbd_multi_world *mw)
{
    for (Shard &s : mw->shards)
        XPBD_TRY(xpbd::frame_snapshot_restore(s.world));
    return XPBD_OK;
}

// One shard's part of an overlap query: its OWNED bodies answer, under their global ids.  Counts first, then lists into a
// buffer of exactly that size; local_ids ascend, so every query's list is ascending in global index.
int shard_overlap(Shard &s, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, std::vector<uint32_t> &offsets,
                  std::vector<xpbd_overlap_hit> &hits)
{
    offsets.assign((size_t)n_queries + 1, 0);
    uint32_t total = 0;
    const int rc = xpbd::overlap_host(s.world, queries, n_queries, flags, offsets.data(), nullptr, 0, &total, s.query_ids.as<uint32_t>());
    if (rc != XPBD_OK && rc != XPBD_E_CAPACITY) // (a count of more than nothing comes back as "no room")
        return rc;
    hits.resize(total);
    if (total == 0)
        return XPBD_OK;
    return xpbd::overlap_host(s.world, queries, n_queries, flags, offsets.data(), hits.data(), total, &total, s.query_ids.as<uint32_t>());
}

int check_usable(const xpbd_multi_world *mw, const char *who)
{
    if (!mw)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (mw->broken)
        return set_error(XPBD_E_HIP, "%s: a collective of this world failed earlier; destroy it on every rank", who);
    return XPBD_OK;
}

// What the scene queries' argument checks (xpbd::check_raycast, xpbd::check_overlap, xpbd::check_sweep) need to know of the world.
xpbd::QueryTarget query_target(const xpbd_multi_world *mw)
{
    return {mw->have_shapes, mw->planned ? mw->n_global : 0u, (uint32_t)mw->shape_radius.size(), "xpbd_multi_world_set_polytopes"};
}

// xpbd_multi_world_raycast(_masked), named `who` in its errors.
int multi_raycast(const char *who, xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, bool masked, uint32_t mask,
                  xpbd_ray_hit *hits)
{
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_raycast(who, query_target(mw), rays, n_rays, flags, hits, true));
    if (!mw->planned) // (a plan over no bodies will do: every ray misses)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    if (n_rays == 0)
        return XPBD_OK;
    // every local shard casts against its owned bodies; one all-gather of the hit records (with every rank's status) over
    // all ranks, then every rank merges the n_ranks rows by the (t, global index) rule of a single world
    LocalStatus st;
    std::vector<std::vector<xpbd_ray_hit>> mine(mw->shards.size(), std::vector<xpbd_ray_hit>(n_rays));
    std::vector<const void *> send;
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        if (st.ok())
            st.keep(xpbd::raycast_host(mw->shards[k].world, rays, n_rays, flags, mine[k].data(), mw->shards[k].query_ids.as<uint32_t>(), masked, mask));
        send.push_back(mine[k].data());
    }
    std::vector<uint8_t> all;
    XPBD_TRY(all_gather_host(mw, send, (size_t)n_rays * sizeof(xpbd_ray_hit), all, st));
    xpbd::merge_ray_hits(all.data(), mw->n_ranks, n_rays, hits);
    return XPBD_OK;
}

// xpbd_multi_world_overlap: every local shard answers for its owned bodies; the counts, the offsets and the hits of every
// rank are gathered and merged per query (xpbd::merge_overlap_lists).
int multi_overlap(xpbd_multi_world *mw, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                  xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
{
    const char *who = "xpbd_multi_world_overlap";
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_overlap(who, query_target(mw), queries, n_queries, flags, offsets, hits, cap, n_out, true));
    if (n_queries == 0) {
        if (n_out)
            *n_out = 0;
        return XPBD_OK;
    }
    const size_t nl = mw->shards.size();
    LocalStatus st;
    std::vector<std::vector<uint32_t>> my_offsets(nl, std::vector<uint32_t>((size_t)n_queries + 1, 0));
    RankLists<xpbd_overlap_hit> lists(nl);
    for (size_t k = 0; k < nl; ++k)
        if (st.ok())
            st.keep(shard_overlap(mw->shards[k], queries, n_queries, flags, my_offsets[k], lists.local[k]));
    XPBD_TRY(gather_counts(mw, st, lists));
    std::vector<const void *> send(nl);
    for (size_t k = 0; k < nl; ++k)
        send[k] = my_offsets[k].data();
    std::vector<uint8_t> all_offsets;
    XPBD_TRY(all_gather_host(mw, send, ((size_t)n_queries + 1) * sizeof(uint32_t), all_offsets, st));
    XPBD_TRY(gather_rows(mw, st, lists));
    uint64_t total = 0;
    for (uint32_t t : lists.counts)
        total += t;
    if (total > 0xFFFFFFFFull)
        return set_error(XPBD_E_INVALID, "%s: %llu hits do not fit the 32-bit offsets", who, (unsigned long long)total);
    *n_out = xpbd::merge_overlap_lists(all_offsets.data(), lists.rows.data(), lists.widest, mw->n_ranks, n_queries, offsets, hits, cap);
    if (*n_out > cap)
        return set_error(XPBD_E_CAPACITY, "%s: %u hits but room for %u", who, *n_out, cap);
    return XPBD_OK;
}

// xpbd_multi_world_sweep: every local shard sweeps against its owned bodies; one all-gather of the hit records, merged by the
// (t, global index) rule of a single world (xpbd::merge_sweep_hits).
int multi_sweep(xpbd_multi_world *mw, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
{
    const char *who = "xpbd_multi_world_sweep";
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_sweep(who, query_target(mw), sweeps, n_sweeps, flags, hits, true));
    if (n_sweeps == 0)
        return XPBD_OK;
    LocalStatus st;
    std::vector<std::vector<xpbd_sweep_hit>> mine(mw->shards.size(), std::vector<xpbd_sweep_hit>(n_sweeps));
    std::vector<const void *> send;
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        if (st.ok())
            st.keep(xpbd::sweep_host(mw->shards[k].world, sweeps, n_sweeps, flags, mine[k].data(), mw->shards[k].query_ids.as<uint32_t>()));
        send.push_back(mine[k].data());
    }
    std::vector<uint8_t> all;
    XPBD_TRY(all_gather_host(mw, send, (size_t)n_sweeps * sizeof(xpbd_sweep_hit), all, st));
    xpbd::merge_sweep_hits(all.data(), mw->n_ranks, n_sweeps, hits);
    return XPBD_OK;
}

// ---- contact reports ----------------------------------------------------------------------------------------------------
void report_clear(xpbd_multi_world *mw)
{
    mw->report_valid = false;
    mw->report_pairs.clear();
    mw->report_points.clear();
    mw->report_events.clear();
    mw->report_prev.clear();
    mw->report_begins = 0;
}

// One shard's part of the frame's report: the pairs whose lower body it owns (the owner holds the other body as well, owned
// or as a ghost), under global ids.  local_ids are ascending, so the shard's list is sorted by global key.
int shard_report(Shard &s, std::vector<xpbd_pair_contact> &pairs, std::vector<xpbd_contact_point> &points)
{
    XPBD_TRY(bind(s));
    if (xpbd_world_body_count(s.world) != s.local_ids.size())
        return set_error(XPBD_E_INVALID, "contact report: shard %u holds %u bodies, its plan %zu", s.rank, xpbd_world_body_count(s.world),
                         s.local_ids.size());
    return xpbd::report_shard(s.world, s.report_owned.as<uint8_t>(), s.report_ids.as<uint32_t>(), pairs, points);
}

// Collective, at the end of an accepted frame: every rank gathers every shard's list, merges them by key (the lists are
// disjoint: a pair belongs to the owner of its lower body) and derives the events from the merged lists, so that owners
// changing at a re-plan do not matter.  Same records as one world over the same bodies.
int capture_report(xpbd_multi_world *mw)
{
    const size_t nl = mw->shards.size();
    LocalStatus st;
    RankLists<xpbd_pair_contact> pairs(nl);
    RankLists<xpbd_contact_point> points(nl);
    for (size_t k = 0; k < nl; ++k)
        if (st.ok())
            st.keep(shard_report(mw->shards[k], pairs.local[k], points.local[k]));
    XPBD_TRY(gather_counts(mw, st, pairs, points));
    XPBD_TRY(gather_rows(mw, st, pairs));
    XPBD_TRY(gather_rows(mw, st, points));
    std::vector<xpbd_pair_contact> merged;
    std::vector<xpbd_contact_point> merged_points;
    std::vector<uint64_t> keys;
    std::vector<xpbd_contact_event> events;
    xpbd::merge_contact_reports(pairs.rows.data(), pairs.widest, pairs.counts.data(), points.rows.data(), points.widest, mw->n_ranks, merged, merged_points, keys);
    mw->report_begins = xpbd::contact_events(keys, mw->report_prev, events);
    mw->report_pairs.swap(merged);
    mw->report_points.swap(merged_points);
    mw->report_events.swap(events);
    mw->report_prev.swap(keys);
    mw->report_valid = true;
    return XPBD_OK;
}

int check_report(const xpbd_multi_world *mw, const char *who)
{
    XPBD_TRY(check_usable(mw, who));
    if (!mw->report_on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_multi_world_set_contact_report)", who);
    if (!mw->report_valid)
        return set_error(XPBD_E_INVALID, "%s: no report: no frame has been stepped since the reports were enabled, the bodies uploaded "
                                         "or a step failed", who);
    return XPBD_OK;
}

} // namespace

extern "C" {

int xpbd_comm_unique_id(uint8_t id[XPBD_COMM_ID_BYTES])
try {
    static_assert(sizeof(ncclUniqueId) == XPBD_COMM_ID_BYTES, "XPBD_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    if (!id)
        return set_error(XPBD_E_INVALID, "xpbd_comm_unique_id: NULL argument");
    const char *why = nullptr;
    const xpbd::RcclApi *api = xpbd::rccl_api(&why);
    if (!api)
        return set_error(XPBD_E_NO_DEVICE, "xpbd_comm_unique_id: RCCL is not available (%s)", why);
    ncclUniqueId u;
    (void)hipGetLastError(); // see rccl_all_gather
    const ncclResult_t r = api->GetUniqueId(&u);
    if (r != ncclSuccess)
        return set_error(XPBD_E_HIP, "ncclGetUniqueId failed: %s", api->GetErrorString(r));
    std::memcpy(id, &u, XPBD_COMM_ID_BYTES);
    return XPBD_OK;
} XPBD_ABI_CATCH

const char *xpbd_comm_library(void) noexcept
try {
    const xpbd::RcclApi *api = xpbd::rccl_api(nullptr);
    return api ? api->path : nullptr;
} catch (...) {
    return nullptr; // (the search for RCCL ran out of host memory)
}

void xpbd_multi_config_default(xpbd_multi_config *cfg) noexcept
{
    if (!cfg)
        return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->n_ranks = 1;
    cfg->n_local = 1;
    cfg->transport = XPBD_TRANSPORT_RCCL;
    cfg->contact_pad = 0.02;
    cfg->halo_margin = 0.5;
    cfg->narrowphase = XPBD_NARROWPHASE_SAT;
}

int xpbd_multi_world_create(xpbd_multi_world **out, const xpbd_multi_config *cfg)
try {
    if (!out || !cfg)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: NULL argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(xpbd_multi_config))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: struct_size %u != %zu", cfg->struct_size, sizeof(xpbd_multi_config));
    if (cfg->reserved != 0)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: reserved must be 0");
    if (cfg->n_ranks == 0 || cfg->n_ranks > 64 || cfg->n_local == 0 || cfg->first_rank + cfg->n_local > cfg->n_ranks || !cfg->devices)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: ranks [%u, %u) of %u (at most 64) and a device list are needed", cfg->first_rank,
                         cfg->first_rank + cfg->n_local, cfg->n_ranks);
    if (cfg->transport != XPBD_TRANSPORT_RCCL && cfg->transport != XPBD_TRANSPORT_LOCAL)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: unknown transport %u", cfg->transport);
    if (cfg->transport == XPBD_TRANSPORT_LOCAL && cfg->n_local != cfg->n_ranks)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: XPBD_TRANSPORT_LOCAL needs every rank in this process (n_local == n_ranks)");
    if (cfg->transport == XPBD_TRANSPORT_RCCL && !cfg->comm_id)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: XPBD_TRANSPORT_RCCL needs comm_id (xpbd_comm_unique_id on one rank, handed to all)");
    if (!(cfg->contact_pad >= 0.0) || !(cfg->halo_margin > 0.0) || cfg->contact_pad > 1.0e6 || cfg->halo_margin > 1.0e6)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: contact_pad %g / halo_margin %g", cfg->contact_pad, cfg->halo_margin);
    if (cfg->flags & ~(XPBD_MULTI_AUTO_REPLAN | XPBD_MULTI_PLAN_THROUGH_DEVICE | XPBD_MULTI_FULL_PLANS))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: unknown flags 0x%x", cfg->flags);
    if (cfg->narrowphase != XPBD_NARROWPHASE_SAT && cfg->narrowphase != XPBD_NARROWPHASE_GJK_EPA)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_create: unknown narrowphase %u", cfg->narrowphase);

    std::unique_ptr<xpbd_multi_world> mw(new xpbd_multi_world); // (deleted on every way out but the last)
    mw->n_ranks = cfg->n_ranks, mw->first_rank = cfg->first_rank, mw->transport = cfg->transport, mw->flags = cfg->flags;
    mw->pad = cfg->contact_pad, mw->margin = cfg->halo_margin, mw->narrowphase = cfg->narrowphase;
    mw->shards = std::vector<Shard>(cfg->n_local);
    if (mw->transport == XPBD_TRANSPORT_RCCL) {
        const char *why = nullptr;
        mw->rccl = xpbd::rccl_api(&why);
        if (!mw->rccl)
            return set_error(XPBD_E_NO_DEVICE, "xpbd_multi_world_create: RCCL is not available (%s)", why);
    }
    for (uint32_t k = 0; k < cfg->n_local; ++k) {
        Shard &s = mw->shards[k];
        s.device = cfg->devices[k];
        s.rank = cfg->first_rank + k;
        s.rccl = mw->rccl;
        xpbd_config wc;
        xpbd_config_default(&wc);
        wc.device = s.device;
        wc.mode = XPBD_MODE_CONTACTS;
        if (int rc = xpbd_world_create(&s.world, &wc))
            return rc;
        if (int rc = xpbd_world_set_contact_pad(s.world, mw->pad))
            return rc;
        if (int rc = xpbd_world_set_narrowphase(s.world, mw->narrowphase))
            return rc;
        s.stream = static_cast<hipStream_t>(xpbd_world_get_stream(s.world));
        hipError_t e = hipSetDevice(s.device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_send, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_recv, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_gathered, hipEventDisableTiming);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.comm_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.disp_host), (size_t)cfg->n_ranks * 16, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s.status_host), 8, hipHostMallocDefault);
        if (e != hipSuccess)
            return set_error(XPBD_E_HIP, "xpbd_multi_world_create: %s", hipGetErrorString(e));
    }
    if (mw->transport == XPBD_TRANSPORT_RCCL) {
        ncclUniqueId id;
        std::memcpy(&id, cfg->comm_id, sizeof id);
        (void)hipGetLastError(); // see rccl_all_gather
        ncclResult_t r = mw->rccl->GroupStart();
        bool device_failed = false;
        int failed_device = 0;
        for (Shard &s : mw->shards) {
            if (r != ncclSuccess)
                break;
            if (hipSetDevice(s.device) != hipSuccess) {
                device_failed = true;
                failed_device = s.device;
                break;
            }
            r = mw->rccl->CommInitRank(&s.comm, (int)mw->n_ranks, id, (int)s.rank);
        }
        const ncclResult_t r_end = mw->rccl->GroupEnd();
        if (device_failed)
            return set_error(XPBD_E_HIP, "xpbd_multi_world_create: hipSetDevice(%d) failed", failed_device);
        if (r == ncclSuccess)
            r = r_end;
        if (r != ncclSuccess)
            return nccl_fail(mw.get(), r, "ncclCommInitRank");
    }
    *out = mw.release();
    return XPBD_OK;
} XPBD_ABI_CATCH

void xpbd_multi_world_destroy(xpbd_multi_world *mw) noexcept { delete mw; }

int xpbd_multi_world_set_polytopes(xpbd_multi_world *mw, const xpbd_polytope *shapes, uint32_t n_shapes)
try {
    if (!mw || !shapes || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_polytopes: NULL argument or no shapes");
    // validated by the first shard before any shard changes; a later failure leaves the world without shapes (and says so)
    mw->have_shapes = false;
    mw->planned = false;
    for (Shard &s : mw->shards)
        if (int rc = xpbd_world_set_polytopes(s.world, shapes, n_shapes))
            return rc;
    mw->shape_radius.assign(n_shapes, 0.0);
    mw->shape_centroid.assign((size_t)3 * n_shapes, 0.0);
    for (uint32_t k = 0; k < n_shapes; ++k) {
        const xpbd_polytope &p = shapes[k];
        for (int a = 0; a < 3; ++a)
            mw->shape_centroid[3 * (size_t)k + a] = p.centroid[a];
        for (uint32_t v = 0; v < p.n_vertices; ++v) {
            double d2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double d = p.vertices_xyz[3 * (size_t)v + a] - p.centroid[a];
                d2 += d * d;
            }
            mw->shape_radius[k] = std::max(mw->shape_radius[k], std::sqrt(d2));
        }
    }
    mw->have_shapes = true;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_max_depenetration_speed(xpbd_multi_world *mw, double speed)
try {
    if (!mw)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_max_depenetration_speed: NULL world");
    for (Shard &s : mw->shards)
        if (int rc = xpbd_world_set_max_depenetration_speed(s.world, speed))
            return rc;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_joint_limits(xpbd_multi_world *mw, const xpbd_joint_limit *limits, uint32_t n_limits)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_joint_limits"));
    if (int rc = xpbd::check_joint_limits("xpbd_multi_world_set_joint_limits", mw->joints.data(), (uint32_t)mw->joints.size(), limits, n_limits))
        return rc;
    mw->limits.assign(limits, limits + n_limits);
    return push_to_shards(mw, push_joint_limits, "joint limits");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_joint_drives(xpbd_multi_world *mw, const xpbd_joint_drive *drives, uint32_t n_drives)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_joint_drives"));
    if (int rc = xpbd::check_joint_drives("xpbd_multi_world_set_joint_drives", mw->joints.data(), (uint32_t)mw->joints.size(), drives, n_drives))
        return rc;
    mw->drives.assign(drives, drives + n_drives);
    return push_to_shards(mw, push_joint_drives, "joint drives");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_collision_filters(xpbd_multi_world *mw, const xpbd_collision_filter *filters, uint32_t n_global, uint32_t flags)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_collision_filters"));
    XPBD_TRY(xpbd::check_per_body("xpbd_multi_world_set_collision_filters", "filters", filters, n_global, mw->n_global, "n_global"));
    if (flags & ~XPBD_FILTER_JOINTED)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_collision_filters: unknown flags 0x%x", flags);
    if (filters && n_global)
        mw->filters.assign(filters, filters + n_global);
    else
        mw->filters.clear();
    mw->filter_flags = flags;
    return push_to_shards(mw, push_collision_filters, "collision filters");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_materials(xpbd_multi_world *mw, const xpbd_material *materials, uint32_t n_global, double ground_friction)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_materials"));
    XPBD_TRY(xpbd::check_per_body("xpbd_multi_world_set_materials", "materials", materials, n_global, mw->n_global, "n_global"));
    if (!(ground_friction >= 0.0))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_materials: ground_friction = %g (must be >= 0, +inf allowed)", ground_friction);
    if (int rc = xpbd::check_materials("xpbd_multi_world_set_materials", materials, n_global))
        return rc;
    if (materials && n_global)
        mw->materials.assign(materials, materials + n_global);
    else
        mw->materials.clear();
    mw->ground_friction = ground_friction;
    return push_to_shards(mw, push_materials, "materials");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_external_wrench(xpbd_multi_world *mw, const uint32_t *indices, uint32_t n, const double *force_xyz,
                                         const double *torque_xyz)
try {
    const char *who = "xpbd_multi_world_set_external_wrench";
    XPBD_TRY(check_usable(mw, who));
    if (n == 0)
        return XPBD_OK;
    if (!force_xyz && !torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: force_xyz and torque_xyz are both NULL", who);
    if (!mw->planned)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, mw->n_global, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "force_xyz", force_xyz, (size_t)n * 3));
    XPBD_TRY(xpbd::check_edit_finite(who, "torque_xyz", torque_xyz, (size_t)n * 3));
    std::vector<uint32_t> slots;
    std::vector<double> force, torque;
    for (Shard &s : mw->shards) {
        slots.clear(), force.clear(), torque.clear();
        for (uint32_t k = 0; k < n; ++k) {
            const int32_t slot = slot_in_shard(s.local_ids, indices ? indices[k] : k);
            if (slot < 0)
                continue;
            slots.push_back((uint32_t)slot);
            if (force_xyz)
                force.insert(force.end(), force_xyz + 3 * (size_t)k, force_xyz + 3 * (size_t)k + 3);
            if (torque_xyz)
                torque.insert(torque.end(), torque_xyz + 3 * (size_t)k, torque_xyz + 3 * (size_t)k + 3);
        }
        if (slots.empty())
            continue;
        if (int rc = xpbd_world_set_external_wrench(s.world, slots.data(), (uint32_t)slots.size(), force_xyz ? force.data() : nullptr,
                                                    torque_xyz ? torque.data() : nullptr))
            return edit_failed(mw, rc, "external forces");
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_apply_impulses(xpbd_multi_world *mw, const xpbd_impulse *list, uint32_t n)
try {
    const char *who = "xpbd_multi_world_apply_impulses";
    XPBD_TRY(check_usable(mw, who));
    if (n == 0)
        return XPBD_OK;
    if (!mw->planned)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    XPBD_TRY(xpbd::check_impulses(who, list, n, mw->n_global));
    std::vector<xpbd_impulse> local;
    for (Shard &s : mw->shards) {
        local.clear();
        for (uint32_t k = 0; k < n; ++k) { // list order kept: the shard's world sorts by slot (stable), which ascends with the global id
            const int32_t slot = slot_in_shard(s.local_ids, list[k].body);
            if (slot < 0)
                continue;
            local.push_back(list[k]);
            local.back().body = (uint32_t)slot;
        }
        if (local.empty())
            continue;
        if (int rc = xpbd_world_apply_impulses(s.world, local.data(), (uint32_t)local.size()))
            return edit_failed(mw, rc, "velocities");
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_upload(xpbd_multi_world *mw, const xpbd_rigid *bodies, const uint32_t *shape_id, uint32_t first_global, uint32_t n_bodies,
                            uint32_t n_global, const xpbd_joint *joints, uint32_t n_joints)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_upload"));
    // Argument errors are found by every rank alike (or are the caller's to agree on): they return before any collective.
    if ((n_bodies && !bodies) || (n_joints && !joints))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_upload: NULL argument");
    if (!mw->have_shapes)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_upload: call xpbd_multi_world_set_polytopes first");
    const Range lo = shard_range(n_global, mw->first_rank, mw->n_ranks), hi = shard_range(n_global, mw->first_rank + (uint32_t)mw->shards.size() - 1, mw->n_ranks);
    if (first_global != lo.first || n_bodies != hi.first + hi.count - lo.first)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_upload: ranks [%u, %u) of %u hand over bodies [%u, %u) of %u, got [%u, %u)", mw->first_rank,
                         mw->first_rank + (uint32_t)mw->shards.size(), mw->n_ranks, lo.first, hi.first + hi.count, n_global, first_global,
                         first_global + n_bodies);
    const size_t n_shapes = mw->shape_radius.size();
    for (uint32_t i = 0; shape_id && i < n_bodies; ++i)
        if (shape_id[i] >= n_shapes)
            return set_error(XPBD_E_INVALID, "xpbd_multi_world_upload: shape_id[%u] = %u >= n_shapes %zu", i, shape_id[i], n_shapes);
    XPBD_TRY(xpbd::check_joints("xpbd_multi_world_upload", joints, n_joints, n_global));
    mw->n_global = n_global, mw->first_global = first_global, mw->n_bodies = n_bodies;
    mw->joints.assign(joints, joints + n_joints);
    mw->limits.clear(); // limits and drives name joints by index: a new upload invalidates them
    mw->drives.clear();
    mw->filters.clear(); // filters name bodies by index
    mw->filter_flags = 0;
    mw->materials.clear(); // and so do materials
    mw->ground_friction = std::numeric_limits<double>::infinity();
    mw->planned = false;
    report_clear(mw);
    mw->cuts_valid = false; // the first plan is a full one
    mw->check_plans = std::getenv("XPBD_MULTI_CHECK_PLANS") != nullptr;
    // the joints at every body (ascending joint index per body): the plans walk the joints of a rank's own bodies only
    mw->joint_lists.build(joints, n_joints, n_global);
    // the largest bounding radius among the bodies handed over here (r_shape + |centroid - com|: a property of the bodies)
    mw->rmax_local = 0.0;
    for (uint32_t i = 0; i < n_bodies; ++i) {
        const uint32_t sid = shape_id ? shape_id[i] : 0u;
        double off2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double d = mw->shape_centroid[3 * (size_t)sid + a] - bodies[i].center_of_mass[a];
            off2 += d * d;
        }
        mw->rmax_local = std::max(mw->rmax_local, mw->shape_radius[sid] + std::sqrt(off2));
    }
    // every shard's slice goes to its device as it is: a world of owned bodies only, which the first plan re-packs
    LocalStatus st;
    for (Shard &s : mw->shards) {
        const Range slice = shard_range(n_global, s.rank, mw->n_ranks);
        s.held_ids.resize(slice.count);
        s.owned_slots_h.resize(slice.count);
        for (uint32_t i = 0; i < slice.count; ++i)
            s.held_ids[i] = slice.first + i, s.owned_slots_h[i] = i;
        s.local_ids = s.held_ids;
        s.ghosts.clear(), s.boundary.clear();
        auto upload = [&]() -> int {
            XPBD_TRY(bind(s));
            if (int rc = xpbd_world_upload_bodies(s.world, bodies + (slice.first - first_global), shape_id ? shape_id + (slice.first - first_global) : nullptr,
                                                  slice.count))
                return rc;
            XPBD_TRY(upload_vector(s.owned_slots, s.owned_slots_h, s.stream));
            XPBD_HIP_TRY(hipStreamSynchronize(s.stream));
            return XPBD_OK;
        };
        if (st.ok())
            st.keep(upload());
    }
    mw->plans = 0;
    mw->rollbacks = 0;
    mw->full_plans = mw->light_plans = 0;
    return make_plan(mw, st);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_replan(xpbd_multi_world *mw)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_replan"));
    if (!mw->planned)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_replan: no bodies uploaded");
    return replan(mw);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_step(xpbd_multi_world *mw, double dt, uint32_t substeps)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_step"));
    // a step that does not finish with a gathered report leaves none, and an empty S_prev for the next one
    struct ReportGuard {
        xpbd_multi_world *mw;
        ~ReportGuard()
        {
            if (!mw->report_valid)
                report_clear(mw);
        }
    } report_guard{mw};
    mw->report_valid = false;
    if (substeps == 0)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_step: substeps must be > 0");
    if (!mw->planned)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_step: no bodies uploaded");
    if (mw->violated)
        return set_error(XPBD_E_HALO, "xpbd_multi_world_step: a body used up its travel allowance within the last frame (%.3g m in margin-equivalent "
                                      "metres, halo_margin %.3g m); that frame was undone -- call xpbd_multi_world_replan (and re-plan more often "
                                      "or raise the margin)", mw->last_displacement, mw->margin);
    ++mw->steps;
    for (int attempt = 0;; ++attempt) {
        LocalStatus st;
        XPBD_TRY(enqueue_frame(mw, dt, substeps, st));
        if (mw->n_ranks == 1) { // no ghosts, nothing to validate: asynchronous after the broadphase (unless reports are gathered)
            if (!st.ok())
                return st.report();
            return mw->report_on ? capture_report(mw) : XPBD_OK;
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
        const double gain = std::max(0.0, moved - mw->last_displacement); // what this frame used up of the allowance
        mw->last_displacement = moved;
        if (moved <= mw->margin) {
            if (mw->report_on) // before a re-plan repacks the shards
                XPBD_TRY(capture_report(mw));
            // pre-emptive: another frame like this one (and half as much again) would outrun the allowance, so re-plan (and
            // re-balance) from the state just reached.  A wrong guess costs a frame: it is undone and run again below.
            if ((mw->flags & XPBD_MULTI_AUTO_REPLAN) && moved + 1.5 * gain > mw->margin)
                XPBD_TRY(replan(mw));
            return XPBD_OK;
        }
        // A body outran its allowance during THIS frame: a remote contact may have been missed in it.  Undo the frame.
        XPBD_TRY(restore_frame(mw));
        ++mw->rollbacks;
        if (!(mw->flags & XPBD_MULTI_AUTO_REPLAN) || attempt == 1) {
            mw->violated = true;
            return set_error(XPBD_E_HALO, "xpbd_multi_world_step: a body used up its travel allowance during this frame (%.3g m in "
                                          "margin-equivalent metres, beyond halo_margin %.3g m%s): remote contacts may have been missed, so the "
                                          "frame was undone -- call xpbd_multi_world_replan and step again%s",
                             moved, mw->margin, attempt ? ", even right after a re-plan" : "",
                             attempt ? " with a larger halo_margin or a shorter frame" : "");
        }
        XPBD_TRY(replan(mw)); // from the restored state; then the same frame again
    }
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_raycast(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits)
try {
    return multi_raycast("xpbd_multi_world_raycast", mw, rays, n_rays, flags, false, 0u, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_raycast_masked(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, uint32_t mask,
                                    xpbd_ray_hit *hits)
try {
    return multi_raycast("xpbd_multi_world_raycast_masked", mw, rays, n_rays, flags, true, mask, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_overlap(xpbd_multi_world *mw, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                             xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
try {
    return multi_overlap(mw, queries, n_queries, flags, offsets, hits, cap, n_out);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_sweep(xpbd_multi_world *mw, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
try {
    return multi_sweep(mw, sweeps, n_sweeps, flags, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_contact_report(xpbd_multi_world *mw, uint32_t enable)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_contact_report"));
    if (enable > 1u)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_contact_report: enable must be 0 or 1, not %u", enable);
    report_clear(mw);
    mw->report_on = false;
    for (Shard &s : mw->shards) // the shards count their touching substeps; their lists are gathered by the step
        XPBD_TRY(xpbd_world_set_contact_report(s.world, enable));
    mw->report_on = enable != 0;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_contact_report_counts(xpbd_multi_world *mw, uint32_t out[4])
try {
    if (mw && !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_contact_report_counts: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_contact_report_counts"));
    out[0] = (uint32_t)mw->report_pairs.size();
    out[1] = (uint32_t)mw->report_points.size();
    out[2] = mw->report_begins;
    out[3] = (uint32_t)mw->report_events.size() - mw->report_begins;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download_pair_contacts(xpbd_multi_world *mw, xpbd_pair_contact *pairs, uint32_t pair_cap, xpbd_contact_point *points,
                                            uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points)
try {
    if (mw && (!n_pairs || !n_points || (!pairs && pair_cap) || (!points && point_cap)))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_pair_contacts: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_download_pair_contacts"));
    const uint32_t k = (uint32_t)mw->report_pairs.size(), total_points = (uint32_t)mw->report_points.size();
    *n_pairs = k;
    *n_points = total_points;
    if (pair_cap)
        std::memcpy(pairs, mw->report_pairs.data(), (size_t)std::min(k, pair_cap) * sizeof(xpbd_pair_contact));
    if (points && point_cap)
        std::memcpy(points, mw->report_points.data(), (size_t)std::min(total_points, point_cap) * sizeof(xpbd_contact_point));
    if (k > pair_cap || (points && total_points > point_cap))
        return set_error(XPBD_E_CAPACITY, "xpbd_multi_world_download_pair_contacts: %u pairs, capacity %u; %u points, capacity %u", k, pair_cap,
                         total_points, point_cap);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download_contact_events(xpbd_multi_world *mw, xpbd_contact_event *out, uint32_t cap, uint32_t *n_out)
try {
    if (mw && (!n_out || (!out && cap)))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_contact_events: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_download_contact_events"));
    const uint32_t total = (uint32_t)mw->report_events.size();
    *n_out = total;
    if (cap)
        std::memcpy(out, mw->report_events.data(), (size_t)std::min(total, cap) * sizeof(xpbd_contact_event));
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_multi_world_download_contact_events: %u events, capacity %u", total, cap);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_synchronize(xpbd_multi_world *mw)
try {
    if (!mw)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_synchronize: NULL world");
    for (Shard &s : mw->shards)
        if (int rc = xpbd_world_synchronize(s.world))
            return rc;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download_owned(xpbd_multi_world *mw, uint32_t *ids, xpbd_rigid *out, uint32_t cap, uint32_t *n_out)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_download_owned"));
    if (!n_out || (cap && (!ids || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_owned: NULL argument");
    if (!mw->planned)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_owned: no bodies uploaded");
    size_t total = 0;
    for (const Shard &s : mw->shards)
        total += s.held_ids.size();
    *n_out = (uint32_t)total;
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_multi_world_download_owned: %zu owned bodies, capacity %u", total, cap);
    std::vector<std::vector<double>> held;
    XPBD_TRY(fetch_owned(mw, held));
    size_t at = 0;
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        const Shard &s = mw->shards[k];
        if (s.held_ids.empty())
            continue;
        std::memcpy(ids + at, s.held_ids.data(), s.held_ids.size() * 4);
        std::memcpy(out + at, held[k].data(), s.held_ids.size() * sizeof(xpbd_rigid));
        at += s.held_ids.size();
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download(xpbd_multi_world *mw, xpbd_rigid *out, uint32_t n)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_download"));
    if (n && !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download: NULL argument");
    if (!mw->planned || n != mw->n_bodies)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download: n = %u but this process handed over %u bodies", n, mw->planned ? mw->n_bodies : 0);
    LocalStatus st;
    std::vector<std::vector<double>> held;
    st.keep(fetch_owned(mw, held));
    const uint32_t lo = mw->first_global, hi = mw->first_global + mw->n_bodies;
    if (mw->shortcut()) { // every owner is here
        if (!st.ok())
            return st.report();
        for (size_t k = 0; k < mw->shards.size(); ++k) {
            const Shard &s = mw->shards[k];
            for (size_t i = 0; i < s.held_ids.size(); ++i)
                std::memcpy(out + (s.held_ids[i] - lo), &held[k][i * kRigid], sizeof(xpbd_rigid));
        }
        return XPBD_OK;
    }
    // one all-gather of every rank's owned bodies (id + state); each process keeps the slice it handed over
    uint32_t cap = 0;
    for (uint32_t c : mw->owned_count)
        cap = std::max(cap, c);
    const size_t row = 4 + (size_t)kRigid * 8, n_local = mw->shards.size();
    std::vector<std::vector<uint8_t>> payload(n_local);
    std::vector<const void *> send(n_local);
    for (size_t k = 0; k < n_local; ++k) {
        const Shard &s = mw->shards[k];
        payload[k].assign((size_t)cap * row, 0xFF);
        for (size_t i = 0; i < s.held_ids.size() && st.ok(); ++i) {
            std::memcpy(&payload[k][i * row], &s.held_ids[i], 4);
            std::memcpy(&payload[k][i * row + 4], &held[k][i * kRigid], kRigid * 8);
        }
        send[k] = payload[k].data();
    }
    std::vector<uint8_t> gathered;
    XPBD_TRY(all_gather_host(mw, send, (size_t)cap * row, gathered, st));
    uint32_t found = 0;
    for (uint32_t r = 0; r < mw->n_ranks; ++r)
        for (uint32_t i = 0; i < mw->owned_count[r]; ++i) {
            const uint8_t *p = gathered.data() + ((size_t)r * cap + i) * row;
            uint32_t g;
            std::memcpy(&g, p, 4);
            if (g >= lo && g < hi) {
                std::memcpy(out + (g - lo), p + 4, sizeof(xpbd_rigid));
                ++found;
            }
        }
    if (found != mw->n_bodies)
        return set_error(XPBD_E_HIP, "xpbd_multi_world_download: %u of the %u bodies of this process came back", found, mw->n_bodies);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_halo_stats(xpbd_multi_world *mw, uint64_t out[6], double *max_displacement)
try {
    if (!mw || !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_halo_stats: NULL argument");
    uint64_t owned = 0, ghosts = 0, boundary = 0;
    for (const Shard &s : mw->shards) {
        owned += s.held_ids.size();
        ghosts += s.ghosts.size();
        boundary += s.boundary.size();
    }
    out[0] = mw->n_global, out[1] = owned, out[2] = ghosts, out[3] = boundary, out[4] = mw->capacity, out[5] = mw->plans;
    if (max_displacement)
        *max_displacement = mw->last_displacement;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_plan_stats(xpbd_multi_world *mw, uint64_t out[12])
try {
    if (!mw || !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_plan_stats: NULL argument");
    uint32_t lo = UINT32_MAX, hi = 0;
    for (uint32_t c : mw->owned_count) {
        lo = std::min(lo, c);
        hi = std::max(hi, c);
    }
    out[0] = mw->plans, out[1] = mw->rollbacks, out[2] = mw->migrated, out[3] = mw->owned_count.empty() ? 0 : lo, out[4] = hi;
    out[5] = mw->steps, out[6] = mw->ns_enqueue, out[7] = mw->ns_wait_broadphase, out[8] = mw->ns_wait_frame, out[9] = mw->ns_plan;
    out[10] = mw->full_plans, out[11] = mw->light_plans;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_owners(xpbd_multi_world *mw, uint8_t *owner, uint32_t n_global)
try {
    if (!mw || !owner)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_owners: NULL argument");
    if (!mw->planned || n_global != mw->n_global)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_owners: n_global = %u but the world has %u bodies", n_global, mw->planned ? mw->n_global : 0);
    if (mw->owner.size() != n_global) {
        // a light plan does not know the owner of every body of the world: ask the ranks what they own (COLLECTIVE then)
        LocalStatus st;
        uint32_t cap = 1;
        for (uint32_t c : mw->owned_count)
            cap = std::max(cap, c);
        const size_t n_local = mw->shards.size();
        std::vector<std::vector<uint32_t>> ids(n_local);
        std::vector<const void *> send(n_local);
        for (size_t k = 0; k < n_local; ++k) {
            ids[k].assign(cap, UINT32_MAX);
            std::copy(mw->shards[k].held_ids.begin(), mw->shards[k].held_ids.end(), ids[k].begin());
            send[k] = ids[k].data();
        }
        std::vector<uint8_t> gathered;
        XPBD_TRY(all_gather_host(mw, send, (size_t)cap * 4, gathered, st));
        std::vector<uint8_t> all(n_global, 0xFF);
        for (uint32_t r = 0; r < mw->n_ranks; ++r)
            for (uint32_t i = 0; i < mw->owned_count[r]; ++i) {
                uint32_t g;
                std::memcpy(&g, gathered.data() + ((size_t)r * cap + i) * 4, 4);
                if (g < n_global)
                    all[g] = (uint8_t)r;
            }
        mw->owner.swap(all);
    }
    std::memcpy(owner, mw->owner.data(), n_global);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_contact_stats(xpbd_multi_world *mw, uint64_t out[3])
try {
    if (!mw || !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_contact_stats: NULL argument");
    out[0] = out[1] = out[2] = 0;
    for (Shard &s : mw->shards) {
        uint64_t one[3] = {0, 0, 0};
        if (int rc = xpbd_world_contact_stats(s.world, one))
            return rc;
        for (int k = 0; k < 3; ++k)
            out[k] += one[k];
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

} // extern "C"
