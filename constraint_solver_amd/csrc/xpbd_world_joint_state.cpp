// xpbd_world_joint_state.cpp -- joint states and drive targets of the single-GPU world: the four entry points, and the way
// back of targets that were set on the device.  Semantics: include/xpbd.h, "Joint STATES and drive TARGETS"; the kernels:
// xpbd_joint_state.hip; the wake requests: Sleep::request_drives.  The host variants stage their arrays in the body edits'
// staging (EditStaging: an index list and a block of values).
#include <vector>

#include "xpbd_world.hpp"

// After xpbd_world_set_drive_targets_device the device holds the truth about the targets.  Whoever re-stages the extras from
// joints.set.drives (xpbd_world_set_joint_limits when SLIDE limits change, a population change) calls this first.
int sync_drive_targets(xpbd_world *w)
{
    JointTables::Extras &e = w->joints.extras;
    if (!e.targets_on_device)
        return XPBD_OK;
    uint32_t n_items = 0;
    for (uint32_t item : e.drive_item_host)
        n_items = item + 1 > n_items ? item + 1 : n_items;
    std::vector<xpbd::ExtraItem> items(n_items);
    XPBD_HIP_TRY(hipMemcpy(items.data(), e.items.ptr, (size_t)n_items * sizeof(xpbd::ExtraItem), hipMemcpyDeviceToHost));
    std::vector<xpbd_joint_drive> &drives = w->joints.set.drives;
    for (size_t d = 0; d < drives.size(); ++d)
        drives[d].target = items[e.drive_item_host[d]].target;
    e.targets_on_device = false;
    return XPBD_OK;
}

extern "C" {

int xpbd_world_joint_states(xpbd_world *w, const uint32_t *joints, uint32_t n, xpbd_joint_state *out)
try {
    const char *who = "xpbd_world_joint_states";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY((xpbd::JointStateTarget{w->joints.csr.n}.check(who, joints, n, out, true)));
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * sizeof(xpbd_joint_state);
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.indices, (size_t)n * 4}, {w->edit.values, bytes}}));
    if (joints)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, joints, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_joint_states(w->arrays(), w->joints.state_tables(), joints ? w->edit.indices.as<uint32_t>() : nullptr, n,
                                           w->edit.values.as<xpbd_joint_state>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->edit.values.ptr, bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_joint_states_device(xpbd_world *w, const uint32_t *dev_joints, uint32_t n, xpbd_joint_state *dev_out)
try {
    const char *who = "xpbd_world_joint_states_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY((xpbd::JointStateTarget{w->joints.csr.n}.check(who, dev_joints, n, dev_out, false)));
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_joint_states(w->arrays(), w->joints.state_tables(), dev_joints, n, dev_out, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_drive_targets(xpbd_world *w, const uint32_t *drives, const double *targets, uint32_t n)
try {
    const char *who = "xpbd_world_set_drive_targets";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    std::vector<xpbd_joint_drive> &resident = w->joints.set.drives;
    XPBD_TRY((xpbd::DriveTargets{resident.data(), (uint32_t)resident.size()}.check(who, drives, targets, n, true)));
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.indices, (size_t)n * 4}, {w->edit.values, (size_t)n * 8}}));
    const uint32_t *dev_drives = drives ? w->edit.indices.as<uint32_t>() : nullptr;
    if (drives)
        XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, drives, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.values.ptr, targets, (size_t)n * 8, hipMemcpyHostToDevice, w->stream));
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request_drives(w, dev_drives, w->edit.values.as<double>(), n));
    XPBD_HIP_TRY(xpbd::launch_drive_targets(w->joints.drive_table(), dev_drives, w->edit.values.as<double>(), n, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    for (uint32_t k = 0; k < n; ++k) // the host copy follows (a device retarget still pending elsewhere stays pending)
        resident[drives ? drives[k] : k].target = targets[k];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_drive_targets_device(xpbd_world *w, const uint32_t *dev_drives, const double *dev_targets, uint32_t n)
try {
    const char *who = "xpbd_world_set_drive_targets_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY((xpbd::DriveTargets{nullptr, (uint32_t)w->joints.set.drives.size()}.check(who, dev_drives, dev_targets, n, false)));
    if (n == 0 || w->joints.set.drives.empty())
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    if (w->sleep.on)
        XPBD_TRY(w->sleep.request_drives(w, dev_drives, dev_targets, n));
    XPBD_HIP_TRY(xpbd::launch_drive_targets(w->joints.drive_table(), dev_drives, dev_targets, n, w->stream));
    w->joints.extras.targets_on_device = true;
    return XPBD_OK;
} XPBD_ABI_CATCH

} // extern "C"
