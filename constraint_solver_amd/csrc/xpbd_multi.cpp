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
// The xpbd_multi*.cpp units (listed in xpbd_multi.hpp) hold what needs a device or a communicator: the shards, the transport,
// the plan-time collectives around the planner (a handful of small all-gathers: cell keys or rims, boundary lists, the records
// of migrating and boundary bodies; no rank holds the global scene), the device half of a plan (re-pack, uploads), settings,
// edits, the frame, the gathers of reports and scene queries and the xpbd_multi_world_* ABI.  The index arithmetic lives in the
// host-only units: every rank's plan, the layout of a shard (local slots, source map, ghost rows, its joints: layout_shard) and
// the re-indexing of joint records in xpbd_plan.hpp; the merges of query hits and of the contact report with its events in
// xpbd_merge.hpp.
// Every plan-time all-gather carries a status word per rank and so does the frame's last one, so a rank that fails locally
// (out of memory, say) still takes part in the collectives and EVERY rank returns an error instead of the others hanging.
//
// Halo validity is checked at the END of every frame, over all ranks: if a body has used up its travel allowance since the
// plan, a remote contact may have been missed IN THAT FRAME -- the frame is undone (the state it started from is kept aside
// on the device), and either re-run after a re-plan (XPBD_MULTI_AUTO_REPLAN) or reported as XPBD_E_HALO with the state of
// the frame's start in place.  A state with possibly missed contacts never reaches the caller.
//
// This unit: what every unit uses (check_usable, shards_disagree), the library of the communicator, create / destroy, the
// shapes, the scalar and the body-indexed settings with their way to the shards (push_*), upload, synchronize, the downloads,
// the owners and the statistics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "xpbd_multi.hpp"

namespace xpbd::multi {

int check_usable(const xpbd_multi_world *mw, const char *who)
{
    if (!mw)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (mw->broken)
        return set_error(XPBD_E_HIP, "%s: a collective of this world failed earlier; destroy it on every rank", who);
    return XPBD_OK;
}

int shards_disagree(xpbd_multi_world *mw, int rc, const char *what) noexcept
{
    mw->broken = true;
    if (!what)
        return set_error(rc, "%s -- the shards were being re-packed: destroy this xpbd_multi_world on every rank", xpbd_last_error());
    return set_error(rc, "%s -- the shards' %s disagree now: destroy this xpbd_multi_world", xpbd_last_error(), what);
}

namespace {

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

int push_joint_limits(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &) { return push_joint_records(mw->settings.limits, s, xpbd_world_set_joint_limits); }

int push_joint_drives(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &) { return push_joint_records(mw->settings.drives, s, xpbd_world_set_joint_drives); }

int push_collision_filters(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    const std::vector<xpbd_collision_filter> local = local_rows(mw->settings.filters, local_ids);
    return xpbd_world_set_collision_filters(s.world, local.empty() ? nullptr : local.data(), (uint32_t)local.size(), mw->settings.filter_flags);
}

int push_materials(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    const std::vector<xpbd_material> local = local_rows(mw->settings.materials, local_ids);
    return xpbd_world_set_materials(s.world, local.empty() ? nullptr : local.data(), (uint32_t)local.size(), mw->settings.ground_friction);
}

// The tail of a setter: the checked and recorded setting goes to every shard of a planned world (the plan hands it over
// otherwise).  Only a device failure fails here, and the shards disagree then.
int push_to_shards(xpbd_multi_world *mw, PushSetting push, const char *what)
{
    if (!mw->plan.planned)
        return XPBD_OK;
    for (Shard &s : mw->shards) {
        int rc = bind(s);
        if (rc == XPBD_OK)
            rc = push(mw, s, s.local_ids);
        if (rc != XPBD_OK)
            return shards_disagree(mw, rc, what);
    }
    return XPBD_OK;
}

} // namespace

// Every body-indexed setting of the world on shard s (its joints are set: the limits name them).  A new setting is added here.
int push_body_settings(const xpbd_multi_world *mw, const Shard &s, const std::vector<uint32_t> &local_ids)
{
    for (PushSetting push : {push_joint_limits, push_joint_drives, push_collision_filters, push_materials})
        XPBD_TRY(push(mw, s, local_ids));
    return XPBD_OK;
}

} // namespace xpbd::multi

using namespace xpbd::multi;

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

    auto mw = std::make_unique<xpbd_multi_world>(); // (destroyed on every way out but the last)
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

void xpbd_multi_world_destroy(xpbd_multi_world *mw) noexcept { std::unique_ptr<xpbd_multi_world> owned(mw); }

int xpbd_multi_world_set_polytopes(xpbd_multi_world *mw, const xpbd_polytope *shapes, uint32_t n_shapes)
try {
    if (!mw || !shapes || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_polytopes: NULL argument or no shapes");
    // compiled once and validated before any shard changes; a later failure leaves the world without shapes (and says so)
    mw->have_shapes = false;
    mw->plan.drop();
    xpbd::ShapeTablesHost t;
    XPBD_TRY(xpbd::compile_polytopes("xpbd_world_set_polytopes", shapes, n_shapes, t));
    for (Shard &s : mw->shards)
        XPBD_TRY(xpbd::install_shape_tables(s.world, t));
    mw->shape_radius = std::move(t.radii); // for the shard planner: max |vertex - centroid| and the centroid per shape
    mw->shape_centroid = std::move(t.centroids);
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
    if (int rc = xpbd::check_joint_limits("xpbd_multi_world_set_joint_limits", mw->settings.joints.data(), (uint32_t)mw->settings.joints.size(), limits, n_limits))
        return rc;
    mw->settings.set_limits(limits, n_limits);
    return push_to_shards(mw, push_joint_limits, "joint limits");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_joint_drives(xpbd_multi_world *mw, const xpbd_joint_drive *drives, uint32_t n_drives)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_joint_drives"));
    if (int rc = xpbd::check_joint_drives("xpbd_multi_world_set_joint_drives", mw->settings.joints.data(), (uint32_t)mw->settings.joints.size(), drives, n_drives))
        return rc;
    mw->settings.set_drives(drives, n_drives);
    return push_to_shards(mw, push_joint_drives, "joint drives");
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_set_collision_filters(xpbd_multi_world *mw, const xpbd_collision_filter *filters, uint32_t n_global, uint32_t flags)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_collision_filters"));
    XPBD_TRY(xpbd::check_per_body("xpbd_multi_world_set_collision_filters", "filters", filters, n_global, mw->n_global, "n_global"));
    if (flags & ~XPBD_FILTER_JOINTED)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_collision_filters: unknown flags 0x%x", flags);
    mw->settings.set_filters(filters, n_global, flags);
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
    mw->settings.set_materials(materials, n_global, ground_friction);
    return push_to_shards(mw, push_materials, "materials");
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
    mw->settings.adopt(joints, n_joints, n_global);
    mw->plan.reset_for_upload();
    mw->report.clear();
    mw->timers.rollbacks = 0;
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
    return make_plan(mw, st);
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
    if (!mw->plan.planned)
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
    if (!mw->plan.planned || n != mw->n_bodies)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download: n = %u but this process handed over %u bodies", n, mw->plan.planned ? mw->n_bodies : 0);
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
    const std::vector<uint32_t> &owned_count = mw->plan.owned_count;
    uint32_t cap = 0;
    for (uint32_t c : owned_count)
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
        for (uint32_t i = 0; i < owned_count[r]; ++i) {
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
    out[0] = mw->n_global, out[1] = owned, out[2] = ghosts, out[3] = boundary, out[4] = mw->plan.capacity, out[5] = mw->plan.plans;
    if (max_displacement)
        *max_displacement = mw->plan.last_displacement;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_plan_stats(xpbd_multi_world *mw, uint64_t out[12])
try {
    if (!mw || !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_plan_stats: NULL argument");
    const PlanState &plan = mw->plan;
    const Timers &t = mw->timers;
    uint32_t lo = UINT32_MAX, hi = 0;
    for (uint32_t c : plan.owned_count) {
        lo = std::min(lo, c);
        hi = std::max(hi, c);
    }
    out[0] = plan.plans, out[1] = t.rollbacks, out[2] = t.migrated, out[3] = plan.owned_count.empty() ? 0 : lo, out[4] = hi;
    out[5] = t.steps, out[6] = t.ns_enqueue, out[7] = t.ns_wait_broadphase, out[8] = t.ns_wait_frame, out[9] = t.ns_plan;
    out[10] = plan.full_plans, out[11] = plan.light_plans;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_owners(xpbd_multi_world *mw, uint8_t *owner, uint32_t n_global)
try {
    if (!mw || !owner)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_owners: NULL argument");
    PlanState &plan = mw->plan;
    if (!plan.planned || n_global != mw->n_global)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_owners: n_global = %u but the world has %u bodies", n_global, plan.planned ? mw->n_global : 0);
    if (plan.owner.size() != n_global) {
        // a light plan does not know the owner of every body of the world: ask the ranks what they own (COLLECTIVE then)
        LocalStatus st;
        uint32_t cap = 1;
        for (uint32_t c : plan.owned_count)
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
            for (uint32_t i = 0; i < plan.owned_count[r]; ++i) {
                uint32_t g;
                std::memcpy(&g, gathered.data() + ((size_t)r * cap + i) * 4, 4);
                if (g < n_global)
                    all[g] = (uint8_t)r;
            }
        plan.owner.swap(all);
    }
    std::memcpy(owner, plan.owner.data(), n_global);
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
