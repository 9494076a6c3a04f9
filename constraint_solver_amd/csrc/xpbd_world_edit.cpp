// xpbd_world_edit.cpp -- what changes resident bodies of the single-GPU world: body edits, population changes (include/xpbd.h,
// "Body EDITS", "Body POPULATION") and the re-planning of a shard of the multi-GPU world on the device (xpbd_internal.h).
#include <algorithm>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "xpbd_world.hpp"
#include "xpbd_body_ops.h"
#include "xpbd_mass_edit.h"
#include "xpbd_population.h"
#include "xpbd_scan.h"

// ---- re-planning a shard of the multi-GPU world on the device (xpbd_multi.cpp) ---------------------------------------------
namespace xpbd {

int halo_cell_keys(xpbd_world *w, const uint32_t *dev_slots, uint32_t n, double edge, int64_t *host_keys, uint32_t *bad_index)
{
    *bad_index = UINT32_MAX;
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() may free a block
    XPBD_HIP_TRY(w->replan.keys.reserve((size_t)n * 8 + 8));
    uint32_t *bad = reinterpret_cast<uint32_t *>(w->replan.keys.as<int64_t>() + n);
    XPBD_HIP_TRY(hipMemsetAsync(bad, 0xFF, 4, w->stream));
    XPBD_HIP_TRY(launch_cell_keys(w->arrays(), dev_slots, n, edge, w->replan.keys.as<int64_t>(), bad, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(host_keys, w->replan.keys.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(bad_index, bad, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

int download_records(xpbd_world *w, const uint32_t *host_slots, uint32_t n, double *out39)
{
    if (n == 0)
        return XPBD_OK;
    for (uint32_t k = 0; k < n; ++k)
        if (host_slots[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd::download_records: slot %u of a world of %u bodies", host_slots[k], w->n);
    if (int rc = bind_device(w))
        return rc;
    constexpr size_t rec = (size_t)(kRigidDoubles + 1) * 8;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->replan.records.reserve((size_t)n * rec));
    XPBD_HIP_TRY(w->replan.src.reserve((size_t)n * 4));
    XPBD_HIP_TRY(hipMemcpyAsync(w->replan.src.ptr, host_slots, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(launch_gather_records(w->arrays(), w->replan.src.as<uint32_t>(), n, w->replan.records.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out39, w->replan.records.ptr, (size_t)n * rec, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

// The world's bodies become: body s = the present body src[s] (src[s] >= 0) or incoming record -src[s] - 1 (39 doubles: an
// xpbd_rigid and its shape id).  Everything stays on the device but the incoming records; otherwise as xpbd_world_upload_bodies
// (joints, history, contact masks and the neighbour lists are dropped).
int repack_bodies(xpbd_world *w, const int32_t *host_src, uint32_t n_new, const double *incoming39, uint32_t n_incoming)
{
    if (!w || (n_new && !host_src) || (n_incoming && !incoming39))
        return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: NULL argument");
    constexpr uint32_t rec = kRigidDoubles + 1;
    uint32_t max_shape_id = w->max_shape_id;
    for (uint32_t s = 0; s < n_new; ++s) {
        const int32_t from = host_src[s];
        if (from >= 0 ? (uint32_t)from >= w->n : (uint32_t)(-(from + 1)) >= n_incoming)
            return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: body %u comes from %d (%u bodies present, %u incoming)", s, from, w->n, n_incoming);
    }
    for (uint32_t k = 0; k < n_incoming; ++k) {
        const double sid = incoming39[(size_t)k * rec + kRigidDoubles];
        if (!(sid >= 0.0) || sid >= (double)w->geom.n_shapes)
            return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: incoming record %u has shape id %g of %u", k, sid, w->geom.n_shapes);
        max_shape_id = std::max(max_shape_id, (uint32_t)sid);
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    // 1. the present bodies in AoS, the new ones gathered from them and from the incoming records
    XPBD_HIP_TRY(w->aos_staging.reserve((size_t)std::max(w->n, 1u) * sizeof(xpbd_rigid)));
    XPBD_HIP_TRY(w->replan.aos.reserve((size_t)std::max(n_new, 1u) * sizeof(xpbd_rigid)));
    XPBD_HIP_TRY(w->replan.shape.reserve((size_t)std::max(n_new, 1u) * 4));
    XPBD_HIP_TRY(w->replan.src.reserve((size_t)std::max(n_new, 1u) * 4));
    XPBD_HIP_TRY(w->replan.incoming.reserve((size_t)std::max(n_incoming, 1u) * rec * 8));
    XPBD_HIP_TRY(launch_soa_to_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    if (n_new)
        XPBD_HIP_TRY(hipMemcpyAsync(w->replan.src.ptr, host_src, (size_t)n_new * 4, hipMemcpyHostToDevice, w->stream));
    if (n_incoming)
        XPBD_HIP_TRY(hipMemcpyAsync(w->replan.incoming.ptr, incoming39, (size_t)n_incoming * rec * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(launch_repack_bodies(w->aos_staging.as<double>(), w->shape_id.as<uint32_t>(), w->replan.src.as<int32_t>(), n_new,
                                      w->replan.incoming.as<double>(), w->replan.aos.as<double>(), w->replan.shape.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the arrays below may move
    // 2. the world takes the new size
    XPBD_TRY(adopt_body_count(w, n_new, max_shape_id));
    // mass properties shared per shape: the bodies that stay kept the property, the incoming ones are checked
    reset_stat_records(w, false, n_incoming);
    for (uint32_t k = 0; k < n_incoming && w->stat_shared; ++k) {
        xpbd_rigid body;
        std::memcpy(&body, incoming39 + (size_t)k * rec, sizeof body);
        absorb_stat_record(w, body, (uint32_t)incoming39[(size_t)k * rec + kRigidDoubles]);
    }
    if (n_new == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipMemsetAsync(w->shape_id.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->shape_id.ptr, w->replan.shape.ptr, (size_t)n_new * 4, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->last_mask.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(launch_aos_to_soa(w->replan.aos.as<double>(), w->arrays(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's buffers are only borrowed
    return XPBD_OK;
}

} // namespace xpbd

extern "C" {

// ---- body edits (include/xpbd.h, "Body EDITS") ---------------------------------------------------------------------------------
namespace {
// Room in the staging buffers of the host variants (growing one frees the old block, which queued work may still use).
int reserve_edit_staging(xpbd_world *w, size_t index_bytes, size_t value_bytes, size_t list_bytes)
{
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.indices, index_bytes}, {w->edit.values, value_bytes}, {w->edit.list, list_bytes}}));
    return XPBD_OK;
}

// The host variants' index list on the device (NULL: 0..n-1 written out, for the kernels that have no such form).
int stage_edit_indices(xpbd_world *w, const uint32_t *indices, uint32_t n, std::vector<uint32_t> &iota)
{
    if (!indices) {
        iota.resize(n);
        for (uint32_t k = 0; k < n; ++k)
            iota[k] = k;
        indices = iota.data();
    }
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    return XPBD_OK;
}
} // namespace

int xpbd_world_set_external_wrench(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *force_xyz, const double *torque_xyz)
try {
    const char *who = "xpbd_world_set_external_wrench";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!force_xyz && !torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: force_xyz and torque_xyz are both NULL", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "force_xyz", force_xyz, (size_t)n * 3));
    XPBD_TRY(xpbd::check_edit_finite(who, "torque_xyz", torque_xyz, (size_t)n * 3));
    XPBD_TRY(bind_device(w));
    const size_t half = (size_t)n * 3 * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, 2 * half, 0));
    double *dev_force = w->edit.values.as<double>(), *dev_torque = dev_force + (size_t)n * 3;
    if (indices)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    if (force_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_force, force_xyz, half, hipMemcpyHostToDevice, w->stream));
    if (torque_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_torque, torque_xyz, half, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_set_wrench(w->arrays(), indices ? w->edit.indices.as<uint32_t>() : nullptr, n, force_xyz ? dev_force : nullptr,
                                         torque_xyz ? dev_torque : nullptr, w->stream));
    if (w->sleep.on) // an edited sleeper wakes with its group at the start of the next step ("SLEEPING")
        XPBD_TRY(w->sleep.request(w, indices ? w->edit.indices.as<uint32_t>() : nullptr, 1, n));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_external_wrench_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_force_xyz,
                                          const double *dev_torque_xyz)
try {
    const char *who = "xpbd_world_set_external_wrench_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!dev_force_xyz && !dev_torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: dev_force_xyz and dev_torque_xyz are both NULL", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (!dev_indices && n != w->n)
        return set_error(XPBD_E_INVALID, "%s: dev_indices == NULL names the bodies 0..n-1, but n = %u and the world holds %u bodies", who, n, w->n);
    if (n > xpbd::kMaxEditEntries)
        return set_error(XPBD_E_INVALID, "%s: n = %u (at most %u entries per call)", who, n, xpbd::kMaxEditEntries);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_set_wrench(w->arrays(), dev_indices, n, dev_force_xyz, dev_torque_xyz, w->stream));
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request(w, dev_indices, 1, n));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_apply_impulses(xpbd_world *w, const xpbd_impulse *list, uint32_t n)
try {
    const char *who = "xpbd_world_apply_impulses";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(xpbd::check_impulses(who, list, n, w->n));
    // the device path wants the entries of a body adjacent; a stable sort keeps their order
    std::vector<xpbd_impulse> sorted(list, list + n);
    std::stable_sort(sorted.begin(), sorted.end(), [](const xpbd_impulse &a, const xpbd_impulse &b) { return a.body < b.body; });
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * sizeof(xpbd_impulse);
    XPBD_TRY(reserve_edit_staging(w, 0, 0, bytes));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.list.ptr, sorted.data(), bytes, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_apply_impulses(w->arrays(), w->edit.list.as<xpbd_impulse>(), n, w->stream));
    if (w->sleep.on) // (an entry's first word is its body)
        XPBD_TRY(w->sleep.request(w, w->edit.list.as<uint32_t>(), sizeof(xpbd_impulse) / 4, n));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // `sorted` is read by the copy
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_apply_impulses_device(xpbd_world *w, const xpbd_impulse *dev_list, uint32_t n)
try {
    const char *who = "xpbd_world_apply_impulses_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!dev_list)
        return set_error(XPBD_E_INVALID, "%s: NULL list", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (reinterpret_cast<uintptr_t>(dev_list) & 15u)
        return set_error(XPBD_E_INVALID, "%s: dev_list must be 16-byte aligned", who);
    if (n > xpbd::kMaxEditEntries)
        return set_error(XPBD_E_INVALID, "%s: n = %u (at most %u entries per call)", who, n, xpbd::kMaxEditEntries);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_apply_impulses(w->arrays(), dev_list, n, w->stream));
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request(w, reinterpret_cast<const uint32_t *>(dev_list), sizeof(xpbd_impulse) / 4, n));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *rows)
try {
    const char *who = "xpbd_world_set_dynamics";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "rows", rows, (size_t)n * xpbd::kDynFields));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kDynFields * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    std::vector<uint32_t> iota;
    XPBD_TRY(stage_edit_indices(w, indices, n, iota));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.values.ptr, rows, bytes, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_import_dynamic(w->arrays(), w->edit.indices.as<uint32_t>(), nullptr, n, w->edit.values.as<double>(), w->stream));
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request(w, w->edit.indices.as<uint32_t>(), 1, n));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_get_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, double *rows)
try {
    const char *who = "xpbd_world_get_dynamics";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, false));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kDynFields * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    std::vector<uint32_t> iota;
    XPBD_TRY(stage_edit_indices(w, indices, n, iota));
    XPBD_HIP_TRY(xpbd::launch_export_dynamic(w->arrays(), w->edit.indices.as<uint32_t>(), n, w->edit.values.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(rows, w->edit.values.ptr, bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

// ---- mass edits (include/xpbd.h, "MASS properties of resident bodies") ----------------------------------------------------------
namespace {
xpbd::MassEditTarget mass_edit_target(const xpbd_world *w)
{
    return xpbd::MassEditTarget{w->n, w->kinematics.list.data(), (uint32_t)w->kinematics.list.size()};
}

// Both variants of xpbd_world_set_mass_properties, after their checks, with the list on the device.  The wake requests come
// first, so that they see the mass properties the bodies rested under (a named fixed body wakes everybody, a named sleeper its
// group).  The contact pipeline's copies of the mass properties are dropped: the per-shape table no longer describes every body of
// a shape, and the per-body records are rebuilt by the next broadphase -- which the split API has to run again too.
int enqueue_mass_edit(xpbd_world *w, const xpbd::MassEditList &list)
{
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request(w, list.indices, 1, list.n));
    XPBD_HIP_TRY(xpbd::launch_set_mass(w->arrays(), w->kinematics.view(), list, w->stream));
    w->stat_shared = false;
    w->stat_rec_valid = false;
    w->bp.have_neighbours = false;
    return XPBD_OK;
}
} // namespace

int xpbd_world_set_mass_properties(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *rows, uint32_t flags)
try {
    const char *who = "xpbd_world_set_mass_properties";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(mass_edit_target(w).check(who, indices, n, rows, flags, true));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kMassRowDoubles * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    if (indices)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.values.ptr, rows, bytes, hipMemcpyHostToDevice, w->stream));
    // (the indices are distinct: no claim pass)
    XPBD_TRY(enqueue_mass_edit(w, xpbd::MassEditList{indices ? w->edit.indices.as<uint32_t>() : nullptr, w->edit.values.as<double>(), n, flags, nullptr}));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_mass_properties_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_rows, uint32_t flags)
try {
    const char *who = "xpbd_world_set_mass_properties_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(mass_edit_target(w).check(who, dev_indices, n, dev_rows, flags, false));
    XPBD_TRY(bind_device(w));
    uint32_t *owner = nullptr;
    if (dev_indices) { // a list may name a body twice: the claim words, one per body
        XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.owner, (size_t)w->stride * 4}}));
        owner = w->edit.owner.as<uint32_t>();
    }
    return enqueue_mass_edit(w, xpbd::MassEditList{dev_indices, dev_rows, n, flags, owner});
} XPBD_ABI_CATCH

int xpbd_world_get_mass_properties(xpbd_world *w, const uint32_t *indices, uint32_t n, double *rows)
try {
    const char *who = "xpbd_world_get_mass_properties";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(mass_edit_target(w).get_check(who, indices, n, rows));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kMassRowDoubles * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    if (indices)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_get_mass(w->arrays(), indices ? w->edit.indices.as<uint32_t>() : nullptr, n, w->edit.values.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(rows, w->edit.values.ptr, bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

// ---- body population (include/xpbd.h, "Body POPULATION") -----------------------------------------------------------------------
namespace {
// Everything a population change replaces, built aside: the body arrays at the new stride, the per-body tables that are on, the
// scratch sized by the stride, and the joint tables.  Only commit_population touches the world, after every allocation, copy
// and launch has succeeded; a stage that is dropped frees its blocks and leaves the previous population in force.
struct PopulationStage {
    uint32_t n = 0, stride = 0;
    DeviceBuffer dyn, stat, shape_id, last_mask, aos_staging, filters, friction, restitution, dyn_alt, rs_start, damping, dp_scratch;
    JointTables joints;
    KinematicBodies kinematics; // (a removal only: the table as it stands stays where nobody leaves)
    bool kinematics_staged = false;
    Sensors sensors; // (only where the world has a table: the flags gathered, the rest of the unit's blocks start over)
    bool sensors_staged = false;
};

// The new body arrays and per-body tables: new body s < n_keep is the present body dev_src[s] (NULL: body s), the n_add bodies
// of `aos` follow.  Device bound, stream idle; enqueues on the world's stream and does not wait.
int stage_bodies(xpbd_world *w, const uint32_t *dev_src, uint32_t n_keep, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n_add,
                 PopulationStage &st)
{
    // (adopt_body_count's bound, before the sum can wrap: this is the other way a world comes by its body count)
    if (n_keep > kMaxBodies || n_add > kMaxBodies - n_keep)
        return set_error(XPBD_E_INVALID, "a world holds at most %u bodies, not %u + %u", kMaxBodies, n_keep, n_add);
    const uint32_t n_new = n_keep + n_add, stride = stride_for(n_new);
    st.n = n_new;
    st.stride = stride;
    XPBD_HIP_TRY(st.dyn.reserve((size_t)xpbd::kDynFields * stride * 8));
    XPBD_HIP_TRY(st.stat.reserve((size_t)xpbd::kStatFields * stride * 8));
    XPBD_HIP_TRY(st.shape_id.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(st.last_mask.reserve((size_t)stride * 4));
    const size_t aos_bytes = (size_t)at_least_one(n_new) * sizeof(xpbd_rigid);
    if (w->aos_staging.bytes < aos_bytes) // (xpbd_world_download_bodies stages n bodies there)
        XPBD_HIP_TRY(st.aos_staging.reserve(aos_bytes));
    XPBD_HIP_TRY(hipMemsetAsync(st.last_mask.ptr, 0, (size_t)stride * 4, w->stream));
    const xpbd::BodyArrays fresh{st.dyn.as<double>(), st.stat.as<double>(), st.shape_id.as<uint32_t>(), stride, n_new};
    XPBD_HIP_TRY(xpbd::launch_population_gather_bodies(w->arrays(), fresh, dev_src, n_keep, w->stream));
    if (n_add) {
        // the appended bodies take k_aos_to_soa's tile path into the same arrays, from slot n_keep on
        double *incoming = (st.aos_staging.ptr ? st.aos_staging : w->aos_staging).as<double>();
        XPBD_HIP_TRY(hipMemcpyAsync(incoming, aos, (size_t)n_add * sizeof(xpbd_rigid), hipMemcpyHostToDevice, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(fresh.shape_id + n_keep, shape_id, (size_t)n_add * 4, hipMemcpyHostToDevice, w->stream));
        const xpbd::BodyArrays tail{fresh.dyn + n_keep, fresh.stat + n_keep, fresh.shape_id + n_keep, stride, n_add};
        XPBD_HIP_TRY(xpbd::launch_aos_to_soa(incoming, tail, w->stream));
    }
    // the per-body tables: a table that is off stays off; an appended body gets the default
    if (w->filters.on) {
        XPBD_HIP_TRY(st.filters.reserve((size_t)at_least_one(n_new) * sizeof(uint2)));
        XPBD_HIP_TRY(xpbd::launch_population_gather_filters(w->ft_filters.as<uint2>(), st.filters.as<uint2>(), dev_src, n_keep, n_new,
                                                            uint2{~0u, ~0u}, w->stream));
    }
    if (w->materials.on) {
        XPBD_HIP_TRY(st.friction.reserve((size_t)at_least_one(n_new) * 8));
        XPBD_HIP_TRY(xpbd::launch_population_gather_doubles(w->mt_friction.as<double>(), st.friction.as<double>(), dev_src, n_keep, n_new,
                                                            std::numeric_limits<double>::infinity(), w->stream));
    }
    if (w->restitution.on) {
        XPBD_HIP_TRY(st.restitution.reserve((size_t)at_least_one(n_new) * 8));
        XPBD_HIP_TRY(xpbd::launch_population_gather_doubles(w->rs_restitution.as<double>(), st.restitution.as<double>(), dev_src, n_keep, n_new, 0.0,
                                                            w->stream));
        if (w->dyn_alt.bytes < (size_t)xpbd::kDynFields * stride * 8) // the velocity pass's scratch follows the stride
            XPBD_HIP_TRY(st.dyn_alt.reserve((size_t)xpbd::kDynFields * stride * 8));
        if (w->rs_start.bytes < (size_t)6 * stride * 8)
            XPBD_HIP_TRY(st.rs_start.reserve((size_t)6 * stride * 8));
    }
    if (w->damping.on) { // the four fields of the rows, each a table of doubles with its own default
        const size_t rs_old = at_least_one(w->n), rs_new = at_least_one(n_new);
        const double defaults[xpbd::kDampingRowFields] = {0.0, 0.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()};
        XPBD_HIP_TRY(st.damping.reserve(xpbd::kDampingRowFields * rs_new * 8));
        for (uint32_t f = 0; f < xpbd::kDampingRowFields; ++f)
            XPBD_HIP_TRY(xpbd::launch_population_gather_doubles(w->dp_rows.as<double>() + f * rs_old, st.damping.as<double>() + f * rs_new, dev_src, n_keep,
                                                                n_new, defaults[f], w->stream));
    }
    if (w->joints.damping.n && w->dp_scratch.bytes < (size_t)6 * stride * 8) // the joint part's scratch follows the stride
        XPBD_HIP_TRY(st.dp_scratch.reserve((size_t)6 * stride * 8));
    if (!w->sensors.host.empty()) { // the sensor flags ("SENSOR bodies"): a survivor keeps its byte, an appended body is no sensor
        XPBD_HIP_TRY(st.sensors.flags.reserve(at_least_one(n_new)));
        XPBD_HIP_TRY(xpbd::launch_sensor_gather(w->sensors.flags.as<uint8_t>(), st.sensors.flags.as<uint8_t>(), dev_src, n_keep, n_new, w->stream));
        st.sensors.host.resize(n_new); // (pageable: the copy returns once the bytes are here)
        if (n_new)
            XPBD_HIP_TRY(hipMemcpyAsync(st.sensors.host.data(), st.sensors.flags.ptr, n_new, hipMemcpyDeviceToHost, w->stream));
        st.sensors_staged = true;
    }
    return XPBD_OK;
}

// Nothing here can fail.  The old blocks leave with the stage.
void commit_population(xpbd_world *w, PopulationStage &st, uint32_t max_shape_id)
{
    auto take = [](DeviceBuffer &mine, DeviceBuffer &fresh) {
        if (fresh.ptr)
            mine = std::move(fresh);
    };
    take(w->dyn, st.dyn);
    take(w->stat, st.stat);
    take(w->shape_id, st.shape_id);
    take(w->last_mask, st.last_mask);
    take(w->aos_staging, st.aos_staging);
    take(w->ft_filters, st.filters);
    take(w->mt_friction, st.friction);
    take(w->rs_restitution, st.restitution);
    take(w->dyn_alt, st.dyn_alt);
    take(w->rs_start, st.rs_start);
    take(w->dp_rows, st.damping);
    take(w->dp_scratch, st.dp_scratch);
    w->joints = std::move(st.joints);
    if (st.kinematics_staged)
        w->kinematics = std::move(st.kinematics);
    if (st.sensors_staged) { // (the callers have waited for the stream: the host copy is complete)
        for (uint8_t flag : st.sensors.host)
            st.sensors.count += flag;
        w->sensors = std::move(st.sensors);
    }
    take_body_count(w, st.n, max_shape_id);
}

// Both variants of xpbd_world_remove_bodies, after their checks: the removal flags are on the device (dev_remove), or
// `indices` still has to be scattered into the world's own flag array (dev_remove == NULL).
int remove_bodies(xpbd_world *w, const uint8_t *dev_remove, const uint32_t *indices, uint32_t n_indices, uint32_t *old_to_new,
                  uint32_t *dev_old_to_new, uint32_t *joint_old_to_new, uint32_t *n_bodies_out)
{
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the scratch below may move, and the old arrays are freed at the end
    const uint32_t n = w->n;
    XPBD_HIP_TRY(w->pop.prefix.reserve(((size_t)n + 1) * 4));
    XPBD_HIP_TRY(w->pop.scan.reserve(xpbd::scan_scratch_bytes(n)));
    XPBD_HIP_TRY(w->pop.map.reserve((size_t)n * 4));
    XPBD_HIP_TRY(w->pop.src.reserve((size_t)n * 4));
    if (!dev_remove) {
        XPBD_HIP_TRY(w->pop.remove.reserve(n));
        XPBD_HIP_TRY(w->pop.indices.reserve((size_t)n_indices * 4));
        XPBD_HIP_TRY(hipMemsetAsync(w->pop.remove.ptr, 0, n, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(w->pop.indices.ptr, indices, (size_t)n_indices * 4, hipMemcpyHostToDevice, w->stream));
        XPBD_HIP_TRY(xpbd::launch_population_mark(w->pop.indices.as<uint32_t>(), n_indices, w->pop.remove.as<uint8_t>(), n, w->stream));
        dev_remove = w->pop.remove.as<uint8_t>();
    }
    XPBD_HIP_TRY(xpbd::launch_population_map(dev_remove, n, w->pop.prefix.as<uint32_t>(), w->pop.scan.as<uint32_t>(), w->pop.map.as<uint32_t>(),
                                             w->pop.src.as<uint32_t>(), w->stream));
    uint32_t n_keep = 0;
    XPBD_HIP_TRY(hipMemcpyAsync(&n_keep, w->pop.prefix.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, w->stream));
    std::vector<uint32_t> map; // on the host only for the caller or for the joint re-index
    if (old_to_new || w->joints.csr.n || w->kinematics.any()) {
        map.resize(n);
        XPBD_HIP_TRY(hipMemcpyAsync(map.data(), w->pop.map.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, w->stream));
    }
    if (dev_old_to_new)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_old_to_new, w->pop.map.ptr, (size_t)n * 4, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    if (n_keep > n)
        return set_error(XPBD_E_HIP, "xpbd_world_remove_bodies: the scan left %u survivors of %u bodies", n_keep, n);
    std::vector<uint32_t> joint_map(w->joints.csr.n);
    if (n_keep == n) { // (the device variant with no flag set) nobody leaves: nothing changes, history and the rest stay
        for (uint32_t j = 0; j < w->joints.csr.n; ++j)
            joint_map[j] = j;
    } else {
        PopulationStage st;
        XPBD_TRY(sync_drive_targets(w)); // the joint tables are re-staged from the host copy
        if (w->joints.csr.n)
            XPBD_TRY(stage_joint_tables(xpbd::remap_joint_set(w->joints.set, map.data(), n, joint_map), n_keep, w->stream, st.joints));
        if (w->kinematics.any()) { // the kinematic table, re-indexed on its host copy next to the joints
            XPBD_TRY(sync_kinematic_targets(w));
            st.kinematics.list = xpbd::remap_kinematics(w->kinematics.list, map.data(), n);
            if (!st.kinematics.list.empty())
                XPBD_TRY(stage_upload(st.kinematics.table, st.kinematics.list.data(), st.kinematics.list.size() * sizeof(xpbd_kinematic)));
            st.kinematics_staged = true;
        }
        XPBD_TRY(stage_bodies(w, w->pop.src.as<uint32_t>(), n_keep, nullptr, nullptr, 0, st));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
        commit_population(w, st, w->max_shape_id); // (max_shape_id stays an upper bound)
        if (n_keep == 0)
            w->stat_shared = false; // as after an upload of no bodies
    }
    if (old_to_new)
        std::memcpy(old_to_new, map.data(), (size_t)n * 4);
    if (joint_old_to_new && !joint_map.empty())
        std::memcpy(joint_old_to_new, joint_map.data(), joint_map.size() * 4);
    if (n_bodies_out)
        *n_bodies_out = n_keep;
    return XPBD_OK;
}
} // namespace

int xpbd_world_remove_bodies(xpbd_world *w, const uint32_t *indices, uint32_t n, uint32_t *old_to_new, uint32_t *joint_old_to_new,
                             uint32_t *n_bodies_out)
try {
    const char *who = "xpbd_world_remove_bodies";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0) { // nothing at all: the maps are the identity
        for (uint32_t i = 0; old_to_new && i < w->n; ++i)
            old_to_new[i] = i;
        for (uint32_t j = 0; joint_old_to_new && j < w->joints.csr.n; ++j)
            joint_old_to_new[j] = j;
        if (n_bodies_out)
            *n_bodies_out = w->n;
        return XPBD_OK;
    }
    if (!indices)
        return set_error(XPBD_E_INVALID, "%s: NULL indices with n = %u", who, n);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    for (uint32_t k = 0; k < n; ++k)
        if (indices[k] >= w->n)
            return set_error(XPBD_E_INVALID, "%s: indices[%u] = %u but the world holds %u bodies", who, k, indices[k], w->n);
    return remove_bodies(w, nullptr, indices, n, old_to_new, nullptr, joint_old_to_new, n_bodies_out);
} XPBD_ABI_CATCH

int xpbd_world_remove_bodies_device(xpbd_world *w, const uint8_t *dev_remove, uint32_t *dev_old_to_new, uint32_t *joint_old_to_new,
                                    uint32_t *n_bodies_out)
try {
    const char *who = "xpbd_world_remove_bodies_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (!dev_remove)
        return set_error(XPBD_E_INVALID, "%s: NULL dev_remove", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    return remove_bodies(w, dev_remove, nullptr, 0, nullptr, dev_old_to_new, joint_old_to_new, n_bodies_out);
} XPBD_ABI_CATCH

int xpbd_world_add_bodies(xpbd_world *w, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n_add, uint32_t *first_index_out)
try {
    const char *who = "xpbd_world_add_bodies";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n_add == 0) {
        if (first_index_out)
            *first_index_out = w->n;
        return XPBD_OK;
    }
    if (!aos || !shape_id)
        return set_error(XPBD_E_INVALID, "%s: NULL aos or shape_id with n_add = %u", who, n_add);
    if (w->geom.n_shapes == 0)
        return set_error(XPBD_E_INVALID, "%s: call xpbd_world_set_shapes first", who);
    if (n_add > std::numeric_limits<uint32_t>::max() - 256u - w->n) // (the stride rounds the count up to a multiple of 256)
        return set_error(XPBD_E_INVALID, "%s: %u + %u bodies exceed what xpbd_world_upload_bodies accepts", who, w->n, n_add);
    uint32_t max_shape_id = w->n ? w->max_shape_id : 0u;
    for (uint32_t i = 0; i < n_add; ++i) {
        if (shape_id[i] >= w->geom.n_shapes)
            return set_error(XPBD_E_INVALID, "%s: shape_id[%u] = %u >= n_shapes %u", who, i, shape_id[i], w->geom.n_shapes);
        max_shape_id = shape_id[i] > max_shape_id ? shape_id[i] : max_shape_id;
    }
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the old arrays are freed at the end
    const uint32_t first = w->n;
    PopulationStage st;
    XPBD_TRY(sync_drive_targets(w)); // the joint tables are re-staged from the host copy
    if (w->joints.csr.n) // the same joints in a world of more bodies: the CSR body -> joints grows
        XPBD_TRY(stage_joint_tables(w->joints.set, first + n_add, w->stream, st.joints));
    XPBD_TRY(stage_bodies(w, nullptr, first, aos, shape_id, n_add, st));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    commit_population(w, st, max_shape_id);
    // mass properties shared per shape: the bodies that stay kept the property, the appended ones are checked (a world that
    // was empty starts over, as an upload does)
    reset_stat_records(w, first == 0, n_add);
    for (uint32_t i = 0; i < n_add && w->stat_shared; ++i)
        absorb_stat_record(w, aos[i], shape_id[i]);
    if (first_index_out)
        *first_index_out = first;
    return XPBD_OK;
} XPBD_ABI_CATCH

} // extern "C"
