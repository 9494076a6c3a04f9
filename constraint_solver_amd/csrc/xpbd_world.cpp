// xpbd_world.cpp -- the single-GPU world of the C ABI in include/xpbd.h: its life, the bodies' way in and out, the body-indexed
// settings with the staging of the joint tables, the history and the step.  The state: xpbd_world.hpp; the shape tables, the
// contact pipeline, reports, scene queries and body edits have units of their own (listed there).
//
// Every ABI call turns into kernel launches.  There is no CPU fallback: without a usable HIP device every compute entry point
// fails with XPBD_E_NO_DEVICE / XPBD_E_HIP.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "xpbd_world.hpp"

constexpr uint32_t kDefaultBlock = 64;

// Do all bodies of a shape share their mass properties bit for bit?  (see stat_shared)  One more body of shape `sid`.
void absorb_stat_record(xpbd_world *w, const xpbd_rigid &body, uint32_t sid)
{
    double v[xpbd::kStatRecDoubles] = {};
    v[0] = body.inverse_mass;
    std::memcpy(v + 1, body.inverse_inertia, 9 * sizeof(double));
    std::memcpy(v + 10, body.center_of_mass, 3 * sizeof(double));
    double *slot = w->stat_shape_host.data() + (size_t)sid * xpbd::kStatRecDoubles;
    if (!w->stat_shape_seen[sid]) {
        std::memcpy(slot, v, sizeof v);
        w->stat_shape_seen[sid] = 1;
    } else if (std::memcmp(slot, v, sizeof v) != 0) {
        w->stat_shared = false;
    }
}

// Before n more bodies are absorbed.  start_over: the bodies before them are gone (an upload, the first bodies of an empty
// world); a changed shape count starts over too, with the property lost.
void reset_stat_records(xpbd_world *w, bool start_over, uint32_t n)
{
    if (start_over || w->stat_shape_seen.size() != w->geom.n_shapes) {
        w->stat_shape_host.assign((size_t)w->geom.n_shapes * xpbd::kStatRecDoubles, 0.0);
        w->stat_shape_seen.assign(w->geom.n_shapes, 0);
        w->stat_shared = start_over && n != 0;
    }
}

// The body arrays hold n_new bodies from now on (the caller made room: stride_for(n_new)): what was derived from the old
// bodies is dropped -- neighbour lists, history, trace, contact masks, frame snapshot and the contact report's state.
void take_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id)
{
    w->bp.have_neighbours = false;
    w->history.length = 0;
    w->history.stepped.clear();
    w->n = n_new;
    w->stride = stride_for(n_new);
    w->stat_rec_valid = false;
    w->max_shape_id = max_shape_id;
    w->stepped = false;
    w->trace_rows = 0;
    w->snapshot.valid = false;
    w->bp.pending = false;
    w->report.reset();
    w->history.sleep_requests.clear();
    w->sleep.fresh = true; // sleeping stays on; every body of the new set is awake with zero counters
    w->sleep.requests = 0;
}

// The settings that name bodies (or the joints between them) by index go back to their defaults.
void drop_body_settings(xpbd_world *w)
{
    w->joints.clear();
    w->filters.clear();
    w->materials.clear();
    w->restitution.clear();
    w->kinematics.clear();
    w->damping.clear();
    w->sensors.clear();
}

// The world takes a new set of n_new bodies (xpbd_world_upload_bodies, xpbd::repack_bodies; device bound, stream idle): room for
// them, and everything that named the old bodies by index or was derived from them is dropped -- the body-indexed settings
// (drop_body_settings) and the derived state (take_body_count).  The callers fill the arrays and see to the per-shape mass
// properties (stat_shape_*), which one resets and the other keeps.  (A population change keeps the settings: it stages its
// arrays itself and calls take_body_count alone.)
int adopt_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id)
{
    // (the stride rounds the count up to a multiple of 256; and no body index can then be XPBD_HIT_TERRAIN or XPBD_NO_HIT)
    static_assert(kMaxBodies - 1u < XPBD_HIT_TERRAIN && XPBD_HIT_TERRAIN < XPBD_NO_HIT, "the scene queries' reserved body indices are no body's");
    if (n_new > kMaxBodies)
        return set_error(XPBD_E_INVALID, "a world holds at most %u bodies, not %u", kMaxBodies, n_new);
    const uint32_t stride = stride_for(n_new);
    XPBD_HIP_TRY(w->dyn.reserve((size_t)xpbd::kDynFields * stride * 8));
    drop_body_settings(w);
    XPBD_HIP_TRY(w->stat.reserve((size_t)xpbd::kStatFields * stride * 8));
    XPBD_HIP_TRY(w->shape_id.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(w->last_mask.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(w->aos_staging.reserve((size_t)at_least_one(n_new) * sizeof(xpbd_rigid)));
    take_body_count(w, n_new, max_shape_id);
    return XPBD_OK;
}

// `bytes` of `values` in a block of its own (no bytes: a block all the same, so that no table of a world with shapes is NULL).
int stage_upload(DeviceBuffer &fresh, const void *values, size_t bytes)
{
    XPBD_HIP_TRY(fresh.reserve(bytes ? bytes : 8));
    if (bytes)
        XPBD_HIP_TRY(hipMemcpy(fresh.ptr, values, bytes, hipMemcpyHostToDevice));
    return XPBD_OK;
}

// A per-body table of a setter: staged in a buffer of its own and moved over `table`, so that a failed allocation or copy
// leaves the previous table in force.  The stream is idle (queued work may still read the present table).
int upload_table(DeviceBuffer &table, const void *values, size_t bytes)
{
    DeviceBuffer fresh;
    XPBD_TRY(stage_upload(fresh, values, bytes));
    table = std::move(fresh);
    return XPBD_OK;
}

namespace {
// ---- the joint tables (JointTables): nothing but these four allocates or copies one -----------------------------------------
// Each fills a fresh part from the host tables of xpbd_population_remap.hpp; the caller moves it in once nothing can fail any
// more, so a failed call leaves the previous tables in force.  An empty part is left without blocks, so every table that is
// copied has at least one element.  The device is bound.
int stage_csr(const xpbd_joint *joints, uint32_t n_joints, const xpbd::JointCsr &csr, uint32_t n_bodies, JointTables::Csr &out)
{
    static_assert(sizeof(xpbd_joint) == sizeof(xpbd::Joint), "xpbd_joint must mirror xpbd::Joint");
    if (n_joints == 0)
        return XPBD_OK;
    XPBD_TRY(stage_upload(out.joints, joints, (size_t)n_joints * sizeof(xpbd::Joint)));
    XPBD_TRY(stage_upload(out.off, csr.off.data(), (size_t)(n_bodies + 1) * 4));
    XPBD_TRY(stage_upload(out.list, csr.list.data(), (size_t)2 * n_joints * 4));
    out.n = n_joints;
    return XPBD_OK;
}

int stage_limits(const xpbd::LimitTables &t, JointTables::Limits &out)
{
    static_assert(sizeof(xpbd_joint_limit) == 72 && sizeof(xpbd_joint_limit) == sizeof(xpbd::JointLimit), "xpbd_joint_limit must mirror xpbd::JointLimit");
    if (t.sorted.empty())
        return XPBD_OK;
    XPBD_TRY(stage_upload(out.limits, t.sorted.data(), t.sorted.size() * sizeof(xpbd::JointLimit)));
    XPBD_TRY(stage_upload(out.limit_off, t.off.data(), t.off.size() * 4));
    out.n_limits = (uint32_t)t.sorted.size();
    return XPBD_OK;
}

// The per-end sums start as zeros, which is what the pair solve reads for a joint that is not listed.
int stage_extras(const xpbd::ExtraTables &t, uint32_t n_joints, hipStream_t stream, JointTables::Extras &out)
{
    static_assert(xpbd::kExtraItemSlideLimit == xpbd::kExtraSlideLimit && sizeof(xpbd::ExtraItem) == sizeof(xpbd::JointExtraItem),
                  "xpbd::ExtraItem must mirror xpbd::JointExtraItem");
    static_assert(sizeof(xpbd_joint_drive) == 80 && sizeof(xpbd_joint_drive) == sizeof(xpbd::JointExtraItem), "xpbd_joint_drive must mirror xpbd::JointExtraItem");
    if (t.list.empty())
        return XPBD_OK;
    const size_t sums = (size_t)2 * n_joints * xpbd::kJointExtraDoubles * 8;
    XPBD_HIP_TRY(out.sums.reserve(sums));
    XPBD_HIP_TRY(hipMemsetAsync(out.sums.ptr, 0, sums, stream));
    XPBD_HIP_TRY(hipStreamSynchronize(stream)); // done before the call returns: a stream the world is given later reads zeros too
    XPBD_TRY(stage_upload(out.joints, t.list.data(), t.list.size() * 4));
    XPBD_TRY(stage_upload(out.slots, t.slots.data(), t.slots.size() * 4));
    XPBD_TRY(stage_upload(out.off, t.off.data(), t.off.size() * 4));
    XPBD_TRY(stage_upload(out.items, t.items.data(), t.items.size() * sizeof(xpbd::ExtraItem)));
    // what the joint states and the drive targets look a joint's / a drive's items up by
    std::vector<uint32_t> joint_slot(n_joints, xpbd::kNoExtraSlot);
    for (size_t k = 0; k < t.list.size(); ++k)
        joint_slot[t.list[k]] = (uint32_t)k;
    XPBD_TRY(stage_upload(out.joint_slot, joint_slot.data(), joint_slot.size() * 4));
    if (!t.drive_item.empty())
        XPBD_TRY(stage_upload(out.drive_item, t.drive_item.data(), t.drive_item.size() * 4));
    out.drive_item_host = t.drive_item;
    out.n_extra_joints = (uint32_t)t.list.size();
    return XPBD_OK;
}

// Stage 7's (mu_l, mu_a) per joint; a list without a nonzero coefficient leaves the part empty, which is what turns the pass off.
int stage_joint_damping(const std::vector<xpbd_joint_damping> &list, uint32_t n_joints, JointTables::Damping &out)
{
    const std::vector<double> table = xpbd::build_joint_damping_table(list, n_joints);
    if (table.empty())
        return XPBD_OK;
    XPBD_TRY(stage_upload(out.table, table.data(), table.size() * sizeof(double)));
    out.n = n_joints;
    return XPBD_OK;
}

} // namespace

// All four from `set` in a world of n_bodies bodies: what the four setters, called in turn, would build.
int stage_joint_tables(xpbd::JointSet set, uint32_t n_bodies, hipStream_t stream, JointTables &out)
{
    out.clear();
    const uint32_t n_joints = (uint32_t)set.joints.size();
    if (n_joints == 0)
        return XPBD_OK;
    xpbd::LimitTables lt = xpbd::build_limit_tables(set.limits.data(), (uint32_t)set.limits.size(), n_joints);
    XPBD_TRY(stage_csr(set.joints.data(), n_joints, xpbd::build_joint_csr(set.joints.data(), n_joints, n_bodies), n_bodies, out.csr));
    XPBD_TRY(stage_limits(lt, out.limits));
    XPBD_TRY(stage_extras(xpbd::build_extra_tables(set.joints, lt.slide, set.drives, n_bodies), n_joints, stream, out.extras));
    XPBD_TRY(stage_joint_damping(set.damping, n_joints, out.damping));
    out.set = std::move(set);
    out.slide_limits = std::move(lt.slide);
    return XPBD_OK;
}

extern "C" {

uint32_t xpbd_abi_version(void) noexcept { return XPBD_ABI_VERSION; }

void xpbd_config_default(xpbd_config *cfg) noexcept
{
    if (!cfg)
        return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0;
    cfg->mode = XPBD_MODE_FUSED;
}

int xpbd_device_count(void)
try {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
        return set_error(XPBD_E_NO_DEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    return n;
} XPBD_ABI_CATCH

int xpbd_world_create(xpbd_world **out, const xpbd_config *cfg)
try {
    if (!out)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: out is NULL");
    *out = nullptr;
    xpbd_config c;
    xpbd_config_default(&c);
    if (cfg) {
        if (cfg->struct_size != sizeof(xpbd_config))
            return set_error(XPBD_E_INVALID, "xpbd_world_create: struct_size %u != %zu", cfg->struct_size,
                             sizeof(xpbd_config));
        c = *cfg;
    }
    if (c.mode != XPBD_MODE_FUSED && c.mode != XPBD_MODE_PER_SUBSTEP && c.mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: unknown mode %u", c.mode);
    if (c.flags & ~XPBD_FLAG_TRACE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: unknown flags 0x%x", c.flags);
    // k_step is compiled with __launch_bounds__(xpbd::kMaxStepBlock): a larger workgroup is a launch failure
    if (c.block_size != 0 && (c.block_size % 64 != 0 || c.block_size > xpbd::kMaxStepBlock))
        return set_error(XPBD_E_INVALID, "xpbd_world_create: block_size %u must be a multiple of 64, <= %u",
                         c.block_size, xpbd::kMaxStepBlock);
    if (c.reserved[0] || c.reserved[1] || c.reserved[2])
        return set_error(XPBD_E_INVALID, "xpbd_world_create: reserved fields must be 0");

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return set_error(XPBD_E_NO_DEVICE, "no HIP device available (%s)",
                         e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (c.device < 0 || c.device >= count)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: device %d out of range [0,%d)", c.device, count);

    std::unique_ptr<xpbd_world> w(new xpbd_world);
    w->device = c.device;
    w->mode = c.mode;
    w->flags = c.flags;
    w->block_size = c.block_size ? c.block_size : kDefaultBlock;
    e = hipSetDevice(w->device);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&w->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess)
        return set_error(XPBD_E_HIP, "xpbd_world_create: stream creation failed: %s", hipGetErrorString(e));
    w->stream = w->own_stream;
    *out = w.release();
    return XPBD_OK;
} XPBD_ABI_CATCH

void xpbd_world_destroy(xpbd_world *w) noexcept { delete w; }

int xpbd_world_upload_bodies(xpbd_world *w, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n)
try {
    if (!w || (!aos && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: NULL argument");
    if (w->geom.n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: call xpbd_world_set_shapes first");
    uint32_t max_shape_id = 0;
    if (shape_id)
        for (uint32_t i = 0; i < n; ++i) {
            if (shape_id[i] >= w->geom.n_shapes)
                return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: shape_id[%u] = %u >= n_shapes %u", i,
                                 shape_id[i], w->geom.n_shapes);
            max_shape_id = shape_id[i] > max_shape_id ? shape_id[i] : max_shape_id;
        }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_TRY(adopt_body_count(w, n, max_shape_id));
    reset_stat_records(w, true, n);
    for (uint32_t i = 0; i < n && w->stat_shared; ++i)
        absorb_stat_record(w, aos[i], shape_id ? shape_id[i] : 0u);
    if (n == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipMemcpyAsync(w->aos_staging.ptr, aos, (size_t)n * sizeof(xpbd_rigid), hipMemcpyHostToDevice,
                                w->stream));
    if (shape_id)
        XPBD_HIP_TRY(hipMemcpyAsync(w->shape_id.ptr, shape_id, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    else
        XPBD_HIP_TRY(hipMemsetAsync(w->shape_id.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->last_mask.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(xpbd::launch_aos_to_soa(w->aos_staging.as<double>(), w->arrays(), w->stream));
    // The caller's buffers are only borrowed for the duration of the call.
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_bodies(xpbd_world *w, xpbd_rigid *aos, uint32_t n)
try {
    if (!w || (!aos && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_bodies: NULL argument");
    if (n != w->n)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_bodies: n = %u but the world holds %u bodies", n, w->n);
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_soa_to_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(aos, w->aos_staging.ptr, (size_t)n * sizeof(xpbd_rigid), hipMemcpyDeviceToHost,
                                w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_body_count(const xpbd_world *w) noexcept { return w ? w->n : 0; }

int xpbd_world_download_frames(xpbd_world *w, double *frames, uint32_t n)
try {
    if (!w || (!frames && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_frames: NULL argument");
    if (n != w->n)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_frames: n = %u but the world holds %u bodies", n, w->n);
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // aos_staging holds n * 38 doubles: room for the n * 7 frame doubles
    XPBD_HIP_TRY(xpbd::launch_body_frames_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(frames, w->aos_staging.ptr, (size_t)n * 7 * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_step(xpbd_world *w, double dt, uint32_t substeps)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_step: NULL world");
    if (substeps == 0) // the reference divides by zero and runs no substep; treat as an argument error
        return set_error(XPBD_E_INVALID, "xpbd_world_step: substeps must be > 0");
    if (w->geom.n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_step: no shapes set");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const double h = dt / (double)substeps; // src/solver.rs:4
    uint32_t *trace = nullptr;
    if (w->flags & XPBD_FLAG_TRACE_CONTACTS) {
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() may free the previous buffer
        XPBD_HIP_TRY(w->trace.reserve((size_t)substeps * w->stride * 4));
        trace = w->trace.as<uint32_t>();
        w->trace_rows = substeps;
    }
    if (w->mode == XPBD_MODE_CONTACTS) {
        if (int rc = step_contacts(w, dt, h, substeps, trace)) {
            w->report.reset();
            return rc;
        }
    } else if (w->mode == XPBD_MODE_FUSED) {
        w->report.reset();
        XPBD_HIP_TRY(xpbd::launch_step(w->arrays(), w->geom.shapes(), h, substeps, w->last_mask.as<uint32_t>(), trace, 0,
                                       w->block_size, w->stream));
    } else {
        w->report.reset();
        for (uint32_t k = 0; k < substeps; ++k)
            XPBD_HIP_TRY(xpbd::launch_step(w->arrays(), w->geom.shapes(), h, 1, w->last_mask.as<uint32_t>(), trace, k,
                                           w->block_size, w->stream));
    }
    w->stepped = true;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_synchronize(xpbd_world *w)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_synchronize: NULL world");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_contacts(xpbd_world *w, xpbd_contact *out, uint32_t cap, uint32_t *n_out)
try {
    if (!w || !n_out || (!out && cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contacts: NULL argument");
    *n_out = 0;
    if (w->n == 0 || !w->stepped)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const uint32_t nb = (w->n + 255) / 256;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->block_counts.reserve((size_t)(nb + 1) * 4));
    XPBD_HIP_TRY(xpbd::launch_contacts_count(w->last_mask.as<uint32_t>(), w->n, w->block_counts.as<uint32_t>(),
                                             w->stream));
    uint32_t total = 0;
    XPBD_HIP_TRY(hipMemcpyAsync(&total, w->block_counts.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    *n_out = total;
    const uint32_t take = total < cap ? total : cap;
    if (take) {
        XPBD_HIP_TRY(w->contacts.reserve((size_t)take * sizeof(xpbd_contact)));
        XPBD_HIP_TRY(xpbd::launch_contacts_emit(w->last_mask.as<uint32_t>(), w->n, w->block_counts.as<uint32_t>(),
                                                w->contacts.as<xpbd_contact>(), take, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(out, w->contacts.ptr, (size_t)take * sizeof(xpbd_contact), hipMemcpyDeviceToHost,
                                    w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_contacts: %u contacts, capacity %u", total, cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_contact_masks(xpbd_world *w, uint32_t *masks, uint32_t substeps, uint32_t n)
try {
    if (!w || !masks)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: NULL argument");
    if (!(w->flags & XPBD_FLAG_TRACE_CONTACTS))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: world created without "
                                         "XPBD_FLAG_TRACE_CONTACTS");
    if (n != w->n || substeps != w->trace_rows)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: asked for %u x %u, last step recorded %u x %u",
                         substeps, n, w->trace_rows, w->n);
    if (n == 0 || substeps == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipMemcpy2DAsync(masks, (size_t)n * 4, w->trace.ptr, (size_t)w->stride * 4, (size_t)n * 4, substeps,
                                  hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_stream(xpbd_world *w, void *hip_stream)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_stream: NULL world");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    w->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : w->own_stream;
    return XPBD_OK;
} XPBD_ABI_CATCH

void *xpbd_world_get_stream(const xpbd_world *w) noexcept { return w ? static_cast<void *>(w->stream) : nullptr; }

int xpbd_world_set_mode(xpbd_world *w, uint32_t mode)
try {
    if (!w || (mode != XPBD_MODE_FUSED && mode != XPBD_MODE_PER_SUBSTEP && mode != XPBD_MODE_CONTACTS))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_mode: bad argument");
    if (w->sleep.on && mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_mode: sleeping is on and needs XPBD_MODE_CONTACTS (xpbd_world_set_sleeping(w, NULL) first)");
    w->mode = mode;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_step_one(xpbd_rigid *rigid, const double *verts_xyz, uint32_t nverts, double dt, uint32_t substeps)
try {
    if (!rigid || !verts_xyz)
        return set_error(XPBD_E_INVALID, "xpbd_step_one: NULL argument");
    // One cached single-body world per host thread (the reference's step is re-entrant and
    // stateless; so is this apart from the cache).
    struct Cache {
        xpbd_world *w = nullptr;
        ~Cache() { xpbd_world_destroy(w); }
    };
    thread_local Cache cache;
    if (!cache.w) {
        xpbd_config cfg;
        xpbd_config_default(&cfg);
        if (int rc = xpbd_world_create(&cache.w, &cfg))
            return rc;
    }
    const uint32_t offsets[2] = {0, nverts};
    if (int rc = xpbd_world_set_shapes(cache.w, verts_xyz, offsets, 1))
        return rc;
    if (int rc = xpbd_world_upload_bodies(cache.w, rigid, nullptr, 1))
        return rc;
    if (int rc = xpbd_world_step(cache.w, dt, substeps))
        return rc;
    return xpbd_world_download_bodies(cache.w, rigid, 1);
} XPBD_ABI_CATCH

// The four joint setters: validate, stage the affected parts aside (stage_csr / stage_limits / stage_extras /
// stage_joint_damping), then commit by moves that cannot fail.  Queued substeps may still read the present tables: the stream is waited for first.
int xpbd_world_set_joints(xpbd_world *w, const xpbd_joint *joints, uint32_t n_joints)
try {
    if (!w || (n_joints && !joints))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joints: NULL argument");
    if (n_joints && w->mode != XPBD_MODE_CONTACTS) // only the contact pipeline projects joints: do not accept and ignore them
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joints: joints need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    XPBD_TRY(xpbd::check_joints("xpbd_world_set_joints", joints, n_joints, w->n));
    xpbd::JointSet set; // (limits, drives and dampers name joints by index: new joints drop them)
    set.joints.assign(joints, joints + n_joints);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables fresh;
    XPBD_TRY(stage_joint_tables(std::move(set), w->n, w->stream, fresh)); // (a slider has an extra entry of its own; no joints: all empty)
    w->joints = std::move(fresh);
    w->sleep.wake_all(true);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_joint_limits(xpbd_world *w, const xpbd_joint_limit *limits, uint32_t n_limits)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_limits: NULL world");
    if (n_limits && w->mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_limits: limits need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    JointTables &J = w->joints;
    XPBD_TRY(xpbd::check_joint_limits("xpbd_world_set_joint_limits", J.set.joints.data(), J.csr.n, limits, n_limits));
    // the SLIDE limits apart (entries of k_joint_extras), the angular ones behind a CSR joint -> limits
    std::vector<xpbd_joint_limit> all(limits, limits + n_limits);
    xpbd::LimitTables lt = xpbd::build_limit_tables(limits, n_limits, J.csr.n);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables::Limits fresh;
    XPBD_TRY(stage_limits(lt, fresh));
    const bool slide_changes = !lt.slide.empty() || !J.slide_limits.empty();
    JointTables::Extras extras;
    if (slide_changes) { // the extras are re-staged from the host copy: targets set on the device come back first
        XPBD_TRY(sync_drive_targets(w));
        XPBD_TRY(stage_extras(xpbd::build_extra_tables(J.set.joints, lt.slide, J.set.drives, w->n), J.csr.n, w->stream, extras));
    }
    J.set.limits = std::move(all);
    J.slide_limits = std::move(lt.slide);
    J.limits = std::move(fresh);
    if (slide_changes)
        J.extras = std::move(extras);
    w->sleep.wake_all(true);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_joint_drives(xpbd_world *w, const xpbd_joint_drive *drives, uint32_t n_drives)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_drives: NULL world");
    if (n_drives && w->mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_drives: drives need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    JointTables &J = w->joints;
    XPBD_TRY(xpbd::check_joint_drives("xpbd_world_set_joint_drives", J.set.joints.data(), J.csr.n, drives, n_drives));
    w->sleep.wake_all(true);
    if (n_drives == 0 && J.set.drives.empty())
        return XPBD_OK;
    std::vector<xpbd_joint_drive> all(drives, drives + n_drives);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables::Extras fresh;
    XPBD_TRY(stage_extras(xpbd::build_extra_tables(J.set.joints, J.slide_limits, all, w->n), J.csr.n, w->stream, fresh));
    J.set.drives = std::move(all);
    J.extras = std::move(fresh); // (with targets_on_device clear: the drives are replaced)
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_joint_damping(xpbd_world *w, const xpbd_joint_damping *list, uint32_t n)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_damping: NULL world");
    if (n && w->mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_damping: joint dampers need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    JointTables &J = w->joints;
    XPBD_TRY((xpbd::DampingTarget{w->n, J.csr.n}.dampers("xpbd_world_set_joint_damping", list, n)));
    w->sleep.wake_all(true);
    if (n == 0 && J.set.damping.empty())
        return XPBD_OK;
    std::vector<xpbd_joint_damping> all(list, list + n);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present table
    JointTables::Damping fresh;
    XPBD_TRY(stage_joint_damping(all, J.csr.n, fresh));
    if (fresh.n) // the joint part's results: follows the stride (a population change grows it)
        XPBD_HIP_TRY(w->dp_scratch.reserve((size_t)6 * (w->stride ? w->stride : 256u) * 8));
    J.set.damping = std::move(all);
    J.damping = std::move(fresh);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_collision_filters(xpbd_world *w, const xpbd_collision_filter *filters, uint32_t n, uint32_t flags)
try {
    static_assert(sizeof(xpbd_collision_filter) == sizeof(uint2), "xpbd_collision_filter must mirror uint2 {group, mask}");
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_collision_filters: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_collision_filters", "filters", filters, n, w->n));
    if (flags & ~XPBD_FILTER_JOINTED)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_collision_filters: unknown flags 0x%x", flags);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued broadphases may still read the present filters
    w->sleep.wake_all(true);
    if (!filters || n == 0) {
        w->filters.clear();
        w->filters.flags = flags;
        return XPBD_OK;
    }
    XPBD_TRY(upload_table(w->ft_filters, filters, (size_t)n * sizeof(uint2)));
    w->filters.on = true;
    w->filters.flags = flags;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_materials(xpbd_world *w, const xpbd_material *materials, uint32_t n, double ground_friction)
try {
    static_assert(sizeof(xpbd_material) == 16, "xpbd_material is {friction, reserved}");
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_materials: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_materials", "materials", materials, n, w->n));
    if (!(ground_friction >= 0.0))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_materials: ground_friction = %g (must be >= 0, +inf allowed)", ground_friction);
    if (int rc = xpbd::check_materials("xpbd_world_set_materials", materials, n))
        return rc;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present coefficients
    w->sleep.wake_all(true);
    const double inf = std::numeric_limits<double>::infinity();
    if ((!materials || n == 0) && ground_friction == inf) { // the default: the contact kernels' plain forms
        w->materials.clear();
        return XPBD_OK;
    }
    // (a finite ground coefficient alone: every body +inf, so that the kernels have one switch, the array)
    std::vector<double> friction(std::max(w->n, 1u), inf);
    for (uint32_t i = 0; materials && i < n; ++i)
        friction[i] = materials[i].friction;
    XPBD_TRY(upload_table(w->mt_friction, friction.data(), friction.size() * sizeof(double)));
    w->materials.on = true;
    w->materials.ground_friction = ground_friction;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_restitution(xpbd_world *w, const double *restitution, uint32_t n, double ground_restitution, double bounce_threshold)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_restitution", "restitution", restitution, n, w->n));
    if (!(ground_restitution >= 0.0 && ground_restitution <= 1.0))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: ground_restitution = %g (must be in [0, 1])", ground_restitution);
    if (!(bounce_threshold >= 0.0 && bounce_threshold <= std::numeric_limits<double>::max()))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: bounce_threshold = %g (must be >= 0 and finite)", bounce_threshold);
    bool any = ground_restitution > 0.0;
    for (uint32_t i = 0; restitution && i < n; ++i) {
        if (!(restitution[i] >= 0.0 && restitution[i] <= 1.0))
            return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: restitution[%u] = %g (must be in [0, 1])", i, restitution[i]);
        any = any || restitution[i] > 0.0;
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present coefficients
    w->sleep.wake_all(true);
    if (!any) { // nothing can bounce: the step runs what it ran before the call
        w->restitution.clear();
        w->restitution.bounce_threshold = bounce_threshold;
        return XPBD_OK;
    }
    std::vector<double> values(std::max(w->n, 1u), 0.0);
    for (uint32_t i = 0; restitution && i < n; ++i)
        values[i] = restitution[i];
    const uint32_t stride = w->stride ? w->stride : 256u;
    XPBD_HIP_TRY(w->dyn_alt.reserve((size_t)xpbd::kDynFields * stride * 8));
    XPBD_HIP_TRY(w->rs_start.reserve((size_t)6 * stride * 8));
    XPBD_TRY(upload_table(w->rs_restitution, values.data(), values.size() * sizeof(double)));
    w->restitution.on = true;
    w->restitution.ground = ground_restitution;
    w->restitution.bounce_threshold = bounce_threshold;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_damping(xpbd_world *w, const xpbd_body_damping *rows, uint32_t n)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_damping: NULL world");
    bool any = false;
    XPBD_TRY((xpbd::DampingTarget{w->n, w->joints.csr.n}.rows("xpbd_world_set_damping", rows, n, &any)));
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present rows
    w->sleep.wake_all(true);
    if (!any) { // every row the default: the step runs what it ran before the call
        w->damping.clear();
        return XPBD_OK;
    }
    // SoA, field by field (xpbd_damping.h)
    const size_t rs = at_least_one(w->n);
    std::vector<double> values(xpbd::kDampingRowFields * rs);
    for (uint32_t i = 0; i < n; ++i) {
        values[0 * rs + i] = rows[i].linear;
        values[1 * rs + i] = rows[i].angular;
        values[2 * rs + i] = rows[i].max_linear_speed;
        values[3 * rs + i] = rows[i].max_angular_speed;
    }
    XPBD_TRY(upload_table(w->dp_rows, values.data(), values.size() * sizeof(double)));
    w->damping.on = true;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_get_damping(xpbd_world *w, xpbd_body_damping *rows, uint32_t n)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_get_damping: NULL world");
    if (n && !rows)
        return set_error(XPBD_E_INVALID, "xpbd_world_get_damping: NULL rows with n = %u", n);
    if (n != w->n)
        return set_error(XPBD_E_INVALID, "xpbd_world_get_damping: n = %u but the world holds %u bodies", n, w->n);
    const double inf = std::numeric_limits<double>::infinity();
    if (!w->damping.on) {
        for (uint32_t i = 0; i < n; ++i)
            rows[i] = xpbd_body_damping{0.0, 0.0, inf, inf};
        return XPBD_OK;
    }
    if (int rc = bind_device(w))
        return rc;
    const size_t rs = at_least_one(w->n);
    std::vector<double> values(xpbd::kDampingRowFields * rs);
    XPBD_HIP_TRY(hipMemcpyAsync(values.data(), w->dp_rows.ptr, values.size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    for (uint32_t i = 0; i < n; ++i)
        rows[i] = xpbd_body_damping{values[0 * rs + i], values[1 * rs + i], values[2 * rs + i], values[3 * rs + i]};
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_terrain(xpbd_world *w, const xpbd_heightfield *hf)
try {
    static_assert(sizeof(xpbd_heightfield) == 48, "xpbd_heightfield is {nx, ny, origin[2], cell[2], heights}");
    const char *who = "xpbd_world_set_terrain";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    size_t samples = 0;
    if (hf) {
        if (hf->nx < 2 || hf->ny < 2)
            return set_error(XPBD_E_INVALID, "%s: %u x %u samples (each must be >= 2)", who, hf->nx, hf->ny);
        samples = (size_t)hf->nx * hf->ny;
        if (samples > XPBD_MAX_TERRAIN_SAMPLES)
            return set_error(XPBD_E_INVALID, "%s: %u x %u samples (at most %u)", who, hf->nx, hf->ny, XPBD_MAX_TERRAIN_SAMPLES);
        if (!hf->heights)
            return set_error(XPBD_E_INVALID, "%s: NULL heights", who);
        for (int a = 0; a < 2; ++a) {
            if (!std::isfinite(hf->origin[a]))
                return set_error(XPBD_E_INVALID, "%s: origin[%d] = %g (must be finite)", who, a, hf->origin[a]);
            if (!(std::isfinite(hf->cell[a]) && hf->cell[a] > 0.0))
                return set_error(XPBD_E_INVALID, "%s: cell[%d] = %g (must be finite and > 0)", who, a, hf->cell[a]);
        }
        for (size_t k = 0; k < samples; ++k)
            if (!std::isfinite(hf->heights[k]))
                return set_error(XPBD_E_INVALID, "%s: heights[%zu] = %g (must be finite)", who, k, hf->heights[k]);
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present table
    w->sleep.wake_all(true);
    if (!hf) {
        w->terrain = xpbd::Terrain{};
        w->tr_planes.release();
        w->tr_heights.release();
        return XPBD_OK;
    }
    // heights and the new table in blocks of their own: the present table stays in force until nothing can fail any more
    xpbd::Terrain t{nullptr, hf->origin[0], hf->origin[1], hf->cell[0], hf->cell[1], hf->nx, hf->ny};
    DeviceBuffer heights, planes;
    XPBD_TRY(stage_upload(heights, hf->heights, samples * sizeof(double)));
    XPBD_HIP_TRY(planes.reserve((size_t)(hf->nx - 1) * (hf->ny - 1) * 8 * sizeof(double)));
    XPBD_HIP_TRY(xpbd::launch_terrain_planes(heights.as<double>(), t, planes.as<double>(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    w->tr_planes = std::move(planes);
    w->tr_heights = std::move(heights);
    t.planes = w->tr_planes.as<double>();
    w->terrain = t;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_sample_terrain(xpbd_world *w, const double *xy, uint32_t n, double *height, double *normal_xyz)
try {
    const char *who = "xpbd_world_sample_terrain";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (!w->terrain.planes)
        return set_error(XPBD_E_INVALID, "%s: the world has no terrain (xpbd_world_set_terrain)", who);
    if (n == 0)
        return XPBD_OK;
    if (!xy || !height)
        return set_error(XPBD_E_INVALID, "%s: NULL xy or height", who);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->terrain_staging.xy, (size_t)n * 2 * 8}, {w->terrain_staging.out, (size_t)n * 4 * 8}}));
    double *dev_height = w->terrain_staging.out.as<double>(), *dev_normal = normal_xyz ? dev_height + n : nullptr;
    XPBD_HIP_TRY(hipMemcpyAsync(w->terrain_staging.xy.ptr, xy, (size_t)n * 2 * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_sample_terrain(w->terrain, w->terrain_staging.xy.as<double>(), n, dev_height, dev_normal, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(height, dev_height, (size_t)n * 8, hipMemcpyDeviceToHost, w->stream));
    if (normal_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(normal_xyz, dev_normal, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_push(xpbd_world *w, uint32_t *index_out)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_push: NULL world");
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_push: no bodies uploaded");
    if (int rc = bind_device(w))
        return rc;
    const size_t slot = w->history_slot_bytes();
    if ((size_t)(w->history.length + 1) * slot > w->history.states.bytes) {
        // grow geometrically into a new block, carrying the old states over (device to device)
        uint32_t capacity = (uint32_t)(w->history.states.bytes / slot);
        capacity = capacity < 8 ? 8 : capacity * 2;
        DeviceBuffer bigger;
        hipError_t e = bigger.reserve((size_t)capacity * slot);
        if (e != hipSuccess)
            return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_world_history_push: %u states of %zu bytes: %s",
                             capacity, slot, hipGetErrorString(e));
        e = hipStreamSynchronize(w->stream);
        if (e == hipSuccess && w->history.length)
            e = hipMemcpy(bigger.ptr, w->history.states.ptr, (size_t)w->history.length * slot, hipMemcpyDeviceToDevice);
        if (e != hipSuccess)
            return set_error(XPBD_E_HIP, "xpbd_world_history_push: carrying %u states over failed: %s", w->history.length, hipGetErrorString(e));
        w->history.states = std::move(bigger); // (the old block goes with `bigger`)
    }
    char *dst = static_cast<char *>(w->history.states.ptr) + (size_t)w->history.length * slot;
    const size_t dyn_bytes = (size_t)xpbd::kDynFields * w->stride * 8;
    XPBD_HIP_TRY(hipMemcpyAsync(dst, w->dyn.ptr, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(dst + dyn_bytes, w->last_mask.ptr, (size_t)w->stride * 4, hipMemcpyDeviceToDevice, w->stream));
    if (w->sleep.on) { // the sleep state behind the masks
        XPBD_TRY(w->sleep.ensure(w));
        XPBD_HIP_TRY(hipMemcpyAsync(dst + dyn_bytes + (size_t)w->stride * 4, w->sleep.state.ptr, Sleep::state_bytes(w->stride), hipMemcpyDeviceToDevice,
                                    w->stream));
    }
    w->history.sleep_requests.push_back((uint8_t)w->sleep.requests);
    w->history.stepped.push_back(w->stepped ? 1 : 0);
    if (index_out)
        *index_out = w->history.length;
    ++w->history.length;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_restore(xpbd_world *w, uint32_t index)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_restore: NULL world");
    if (index >= w->history.length)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_restore: state %u of %u", index, w->history.length);
    if (int rc = bind_device(w))
        return rc;
    const size_t slot = w->history_slot_bytes();
    const char *src = static_cast<const char *>(w->history.states.ptr) + (size_t)index * slot;
    const size_t dyn_bytes = (size_t)xpbd::kDynFields * w->stride * 8;
    XPBD_HIP_TRY(hipMemcpyAsync(w->dyn.ptr, src, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->last_mask.ptr, src + dyn_bytes, (size_t)w->stride * 4, hipMemcpyDeviceToDevice, w->stream));
    if (w->sleep.on) {
        XPBD_TRY(w->sleep.ensure(w));
        XPBD_HIP_TRY(hipMemcpyAsync(w->sleep.state.ptr, src + dyn_bytes + (size_t)w->stride * 4, Sleep::state_bytes(w->stride), hipMemcpyDeviceToDevice,
                                    w->stream));
        w->sleep.requests = w->history.sleep_requests[index];
    }
    w->stepped = w->history.stepped[index] != 0;
    w->bp.have_neighbours = false;
    w->report.reset();
    w->trace_rows = 0; // the per-substep trace belongs to the step call that was overwritten
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_truncate(xpbd_world *w, uint32_t length)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_truncate: NULL world");
    if (length > w->history.length)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_truncate: length %u > %u", length, w->history.length);
    w->history.length = length;
    w->history.stepped.resize(length);
    w->history.sleep_requests.resize(length);
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_history_length(const xpbd_world *w) noexcept { return w ? w->history.length : 0; }

} // extern "C"
