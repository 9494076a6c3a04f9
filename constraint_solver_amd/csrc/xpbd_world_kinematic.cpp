// xpbd_world_kinematic.cpp -- kinematic bodies of the single-GPU world: KinematicBodies (xpbd_world.hpp), the four entry
// points, and the way back of rows that were set on the device.  Semantics: include/xpbd.h, "KINEMATIC bodies"; the kernels:
// xpbd_kinematic.hip; where a frame applies the table: step_contacts / substep_contacts (xpbd_world_contacts.cpp).  The host
// variants stage their arrays in the body edits' staging (EditStaging: an index list and a block of values).
#include <vector>

#include "xpbd_world.hpp"

// After xpbd_world_set_kinematic_targets_device the device holds the truth about the rows.  Whoever re-stages the table from
// kinematics.list (a population change) calls this first.
int sync_kinematic_targets(xpbd_world *w)
{
    KinematicBodies &kin = w->kinematics;
    if (!kin.targets_on_device || kin.list.empty())
        return XPBD_OK;
    std::vector<xpbd_kinematic> now(kin.list.size());
    XPBD_HIP_TRY(hipMemcpy(now.data(), kin.table.ptr, now.size() * sizeof(xpbd_kinematic), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < now.size(); ++k) // (body and mode are never written on the device)
        for (uint32_t c = 0; c < xpbd::kKinematicRowDoubles; ++c)
            kin.list[k].linear[c] = now[k].linear[c];
    kin.targets_on_device = false;
    return XPBD_OK;
}

extern "C" {

int xpbd_world_set_kinematics(xpbd_world *w, const xpbd_kinematic *list, uint32_t n)
try {
    const char *who = "xpbd_world_set_kinematics";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    const xpbd::KinematicTarget target{w->n};
    XPBD_TRY(target.check(who, list, n));
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued work may still read the present table
    if (n == 0) {
        w->kinematics.clear();
        return XPBD_OK;
    }
    // the new table aside; the mass properties of the bodies it names, gathered through it
    DeviceBuffer fresh, mass_dev;
    XPBD_TRY(stage_upload(fresh, list, (size_t)n * sizeof(xpbd_kinematic)));
    XPBD_HIP_TRY(mass_dev.reserve((size_t)n * xpbd::kKinematicMassDoubles * 8));
    std::vector<double> mass((size_t)n * xpbd::kKinematicMassDoubles);
    XPBD_HIP_TRY(xpbd::launch_kinematic_mass(w->arrays(), xpbd::KinematicTable{fresh.as<xpbd_kinematic>(), n}, mass_dev.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(mass.data(), mass_dev.ptr, mass.size() * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_TRY(target.fixed_check(who, list, n, mass.data()));
    std::vector<xpbd_kinematic> host(list, list + n);
    w->kinematics.list.swap(host); // nothing can fail any more
    w->kinematics.table = std::move(fresh);
    w->kinematics.targets_on_device = false;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_kinematic_targets(xpbd_world *w, const uint32_t *entries, const double *rows, uint32_t n)
try {
    const char *who = "xpbd_world_set_kinematic_targets";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    std::vector<xpbd_kinematic> &resident = w->kinematics.list;
    XPBD_TRY((xpbd::KinematicTargets{resident.data(), (uint32_t)resident.size()}.check(who, entries, rows, n, true)));
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    const size_t row_bytes = (size_t)n * xpbd::kKinematicRowDoubles * 8;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.indices, (size_t)n * 4}, {w->edit.values, row_bytes}}));
    const uint32_t *dev_entries = entries ? w->edit.indices.as<uint32_t>() : nullptr;
    if (entries)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, entries, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.values.ptr, rows, row_bytes, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_kinematic_retarget(w->kinematics.view(), dev_entries, w->edit.values.as<double>(), n, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    for (uint32_t k = 0; k < n; ++k) // the host copy follows (a device retarget still pending elsewhere stays pending)
        for (uint32_t c = 0; c < xpbd::kKinematicRowDoubles; ++c)
            resident[entries ? entries[k] : k].linear[c] = rows[(size_t)k * xpbd::kKinematicRowDoubles + c];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_kinematic_targets_device(xpbd_world *w, const uint32_t *dev_entries, const double *dev_rows, uint32_t n)
try {
    const char *who = "xpbd_world_set_kinematic_targets_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY((xpbd::KinematicTargets{nullptr, (uint32_t)w->kinematics.list.size()}.check(who, dev_entries, dev_rows, n, false)));
    if (n == 0 || !w->kinematics.any())
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_kinematic_retarget(w->kinematics.view(), dev_entries, dev_rows, n, w->stream));
    w->kinematics.targets_on_device = true;
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_kinematic_count(const xpbd_world *w) noexcept { return w ? (uint32_t)w->kinematics.list.size() : 0u; }

} // extern "C"
