// xpbd_multi.hpp -- the multi-GPU world behind the C ABI: its state, the owners of the parts that have an invariant, and what
// the units that implement it share (not installed; no .hip file includes it).  The overview is in xpbd_multi.cpp.
//
//   xpbd_multi.cpp            create/destroy, shapes, the scalar and body-indexed setters with push_*, upload, download, stats
//   xpbd_multi_transport.cpp  the all-gathers (RCCL, in-process), all_gather_host, breaking the transport
//   xpbd_multi_plan.cpp       the device half of a plan and its collectives, PlanState's methods, re-plan
//   xpbd_multi_frame.cpp      a shard's frame, the frame on every shard, its end, undoing it; xpbd_multi_world_step
//   xpbd_multi_query.cpp      the gathers of the scene queries
//   xpbd_multi_report.cpp     WorldReport, gathering the contact report, the report entry points
//   xpbd_multi_edit.cpp       body edits
//   xpbd_multi_workers.hpp    Barrier, LocalStatus, ShardJob, FrameWorkers (host only)
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/xpbd.h"
#include "xpbd_internal.h"
#include "xpbd_multi_workers.hpp"
#include "xpbd_plan.hpp"
#include "xpbd_rccl.h"

struct xpbd_multi_world;

// Everything here but xpbd_multi_world itself stays inside the library: the units share it, nobody outside links to it.
#pragma GCC visibility push(hidden)

namespace xpbd::multi {

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

// Body-indexed settings: the world's copy under GLOBAL indices (push_body_settings hands every shard its rows).  Each names
// bodies, or the joints between them, by index, so new bodies end all of them: adopt() is the only code that replaces the
// joints, and a new setting adds its default there.  The set_* methods record what a setter has checked.
struct BodySettings {
    std::vector<xpbd_joint> joints;
    std::vector<xpbd_joint_limit> limits; // xpbd_multi_world_set_joint_limits: GLOBAL joint indices
    std::vector<xpbd_joint_drive> drives; // xpbd_multi_world_set_joint_drives: GLOBAL joint indices
    std::vector<xpbd_collision_filter> filters; // xpbd_multi_world_set_collision_filters: [n_global] or empty (none)
    uint32_t filter_flags = 0;
    std::vector<xpbd_material> materials; // xpbd_multi_world_set_materials: [n_global] or empty (every body +inf)
    double ground_friction = std::numeric_limits<double>::infinity();
    JointLists joint_lists; // the joints at every body (indices into `joints`, ascending)

    void adopt(const xpbd_joint *new_joints, uint32_t n_joints, uint32_t n_global)
    {
        joints.assign(new_joints, new_joints + n_joints);
        set_limits(nullptr, 0); // limits and drives name joints by index: a new upload invalidates them
        set_drives(nullptr, 0);
        set_filters(nullptr, 0, 0); // filters name bodies by index
        set_materials(nullptr, 0, std::numeric_limits<double>::infinity()); // and so do materials
        // the joints at every body (ascending joint index per body): the plans walk the joints of a rank's own bodies only
        joint_lists.build(new_joints, n_joints, n_global);
    }
    void set_limits(const xpbd_joint_limit *rows, uint32_t n) { limits.assign(rows, rows + n); }
    void set_drives(const xpbd_joint_drive *rows, uint32_t n) { drives.assign(rows, rows + n); }
    void set_filters(const xpbd_collision_filter *rows, uint32_t n, uint32_t flags) // (no rows: none)
    {
        filters.assign(rows, rows + (rows ? n : 0));
        filter_flags = flags;
    }
    void set_materials(const xpbd_material *rows, uint32_t n, double ground)
    {
        materials.assign(rows, rows + (rows ? n : 0));
        ground_friction = ground;
    }
};

// The plan in force (xpbd_multi_plan.cpp): is there one, is it still good, and what the next one builds on.  Only the methods
// move it.  planned: every shard is packed by one plan.  violated: a body outran its allowance and the frame was undone; the
// next plan clears it.  plan_torn: a plan stopped while the shards were being re-packed (make_plan breaks the world then).
// cuts_valid: `cuts` and `cut_axes` are a full plan's, the light plans keep them.
struct PlanState {
    bool planned = false, violated = false, plan_torn = false, cuts_valid = false, check_plans = false;
    uint32_t capacity = 1; // rows per rank of the per-substep all-gather
    double cell_edge = 0.0;
    double last_displacement = 0.0; // the largest fraction of its travel allowance any body had used at the last check, times halo_margin
    uint32_t balance_most = 0, balance_least = 0; // most / fewest bodies of a rank right after the last full plan
    std::vector<uint8_t> owner;        // [n_global] as of the last plan
    std::vector<uint32_t> owned_count; // [n_ranks]
    std::vector<Cut> cuts;             // the cuts of the last full plan, kept by the light plans between (cuts_valid)
    int cut_axes[3] = {0, 1, 2};       // ... over slab keys packed in this order of the axes
    std::vector<int32_t> slot_of;      // [n_global] scratch of a plan: local slot of a body, -1 outside the shard being built
    uint64_t plans = 0, full_plans = 0, light_plans = 0;

    uint32_t rows_per_rank() const { return capacity; }
    void reset_for_upload();                  // new bodies: no plan, no cuts (the first plan is a full one), the counters start over
    void drop() { planned = false; }          // new shapes: the shards have to be packed again
    void accept(uint32_t rows, double edge);  // every rank has left a plan: it is in force
    void accept_full(std::vector<uint8_t> &new_owner, std::vector<uint32_t> &new_count); // ... and it was a full / a light one
    void accept_light(std::vector<uint32_t> &new_count);
    void tear() { plan_torn = true; }
    void frame_moved(double moved) { last_displacement = moved; } // the end of a frame
    void violate() { violated = true; }
};

// Contact reports (xpbd_multi_world_set_contact_report; xpbd_multi_report.cpp): the whole world's report of the last frame,
// gathered on every rank when the frame has been accepted (before a re-plan repacks the shards), and the touching pairs of the
// frame before it.  Only the methods move it.
struct WorldReport {
    bool on = false, valid = false;
    std::vector<xpbd_pair_contact> pairs;
    std::vector<xpbd_contact_point> points;
    std::vector<xpbd_contact_event> events;
    std::vector<uint64_t> prev; // keys (a << 32 | b) of the previous frame's touching pairs; empty: S_prev is empty
    uint32_t begins = 0;

    void clear();
    void enable(bool enable); // (either way what was gathered goes)
    // The merged lists of an accepted frame and their keys: the events against the frame before, then `keys` is that frame.
    void accept(std::vector<xpbd_pair_contact> &merged, std::vector<xpbd_contact_point> &merged_points, std::vector<uint64_t> &keys);
    // A step that does not finish with a gathered report leaves none, and an empty S_prev for the next one.
    struct StepGuard {
        WorldReport &r;
        explicit StepGuard(WorldReport &report) : r(report) { r.valid = false; }
        StepGuard(const StepGuard &) = delete;
        StepGuard &operator=(const StepGuard &) = delete;
        ~StepGuard()
        {
            if (!r.valid)
                r.clear();
        }
    };
};

// What xpbd_multi_world_plan_stats reports beside the plan counters.
struct Timers {
    uint64_t steps = 0, rollbacks = 0, migrated = 0, ns_enqueue = 0, ns_wait_broadphase = 0, ns_wait_frame = 0, ns_plan = 0;
};

} // namespace xpbd::multi

#pragma GCC visibility pop

struct xpbd_multi_world {
    uint32_t n_ranks = 1, first_rank = 0, transport = XPBD_TRANSPORT_RCCL, flags = 0, narrowphase = XPBD_NARROWPHASE_SAT;
    double pad = 0.02, margin = 0.5;
    std::vector<xpbd::multi::Shard> shards;
    const xpbd::RcclApi *rccl = nullptr;
    bool have_shapes = false, broken = false;
    std::vector<double> shape_radius, shape_centroid; // per shape: max |vertex - centroid|, centroid xyz
    uint32_t n_global = 0, first_global = 0, n_bodies = 0;
    double rmax_local = 0.0; // largest bounding radius (r_shape + |centroid - com|) among the bodies this process handed over
    xpbd::multi::BodySettings settings;
    xpbd::multi::PlanState plan;
    xpbd::multi::WorldReport report;
    xpbd::multi::Timers timers;
    // One enqueueing thread per local shard (n_local > 1), started by the first step.  Declared after `shards`, so destroyed
    // before them: the threads are joined while every Shard they drive is still there.  No destructor body is needed.
    xpbd::multi::FrameWorkers workers;
    bool all_local() const { return shards.size() == n_ranks; }
    bool shortcut() const { return all_local() && !(flags & XPBD_MULTI_PLAN_THROUGH_DEVICE); } // plan-time gathers are memcpys
    xpbd::multi::Shard *local_shard(uint32_t rank) { return rank >= first_rank && rank < first_rank + shards.size() ? &shards[rank - first_rank] : nullptr; }
};

#pragma GCC visibility push(hidden)

namespace xpbd::multi {

inline uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- xpbd_multi.cpp ---------------------------------------------------------------------------------------------------------
int check_usable(const xpbd_multi_world *mw, const char *who);
// The shards have stopped being one world: a setting or an edit (`what`) reached some of them and failed on the next, or
// (what == NULL) a plan stopped while it re-packed them.  Every later call on the world fails.
int shards_disagree(xpbd_multi_world *mw, int rc, const char *what) noexcept;
int push_body_settings(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids);

// ---- xpbd_multi_transport.cpp -----------------------------------------------------------------------------------------------
int bind(const Shard &s);
int nccl_fail(const xpbd_multi_world *mw, ncclResult_t r, const char *what);
int transport_broken(xpbd_multi_world *mw, int rc) noexcept;
int rccl_all_gather(xpbd_multi_world *mw, Shard &s, const void *send, void *recv, size_t bytes, hipStream_t stream);
int local_send(Shard &s, hipStream_t stream);
int local_copy(xpbd_multi_world *mw, Shard &s, DeviceBuffer Shard::*send, void *recv, size_t bytes, hipStream_t stream);
int local_release(xpbd_multi_world *mw, Shard &s, hipStream_t stream);
int all_gather_host(xpbd_multi_world *mw, const std::vector<const void *> &send, size_t bytes, std::vector<uint8_t> &out, LocalStatus &status);

// ---- xpbd_multi_plan.cpp ----------------------------------------------------------------------------------------------------
int make_plan(xpbd_multi_world *mw, LocalStatus &st);
int replan(xpbd_multi_world *mw);
int fetch_owned(xpbd_multi_world *mw, std::vector<std::vector<double>> &held);

// ---- xpbd_multi_report.cpp --------------------------------------------------------------------------------------------------
int capture_report(xpbd_multi_world *mw);

// Closes the function-try-block of every xpbd_multi_world_* call (but create): an exception leaves the shards in an unknown
// state and maybe the peers inside a collective, so it breaks the transport (see XPBD_ABI_CATCH).
#define XPBD_MULTI_ABI_CATCH \
    catch (...) { return ::xpbd::multi::transport_broken(mw, xpbd::abi_exception(__func__)); }

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

} // namespace xpbd::multi

#pragma GCC visibility pop
