// xpbd_joint_state.h -- joint STATES and drive TARGETS (EXTENSION): launchers for xpbd_joint_state.hip.  Semantics:
// include/xpbd.h, "Joint STATES and drive TARGETS".  Neither kernel is part of the step: one reads the bodies and the joint
// tables, the other writes the `target` word of resident extras items.
#pragma once

#include "xpbd_contacts.h"

namespace xpbd {

constexpr uint32_t kNoExtraSlot = 0xFFFFFFFFu; // JointStateTables::extra_slot of a joint without extras

// The joint tables of a world as k_joint_states reads them (a part the world does not hold is NULL).
struct JointStateTables {
    const Joint *joints;
    uint32_t n_joints;
    const JointLimit *limits;          // the angular limits behind the CSR joint -> limits (the pair solve's table)
    const uint32_t *limit_off;         // [n_joints + 1]; NULL: no angular limits
    const uint32_t *extra_slot;        // [n_joints] joint -> its slot in extra_joints, kNoExtraSlot: none; NULL: no extras at all
    const uint32_t *extra_off;         // [n_extra_joints + 1]
    const JointExtraItem *extra_items; // the SLIDE limit first, then the drives in the caller's order
};

// The drives of a world as k_drive_targets and the sleep unit's launch_sleep_request_drives read them.
struct DriveTable {
    JointExtraItem *items;      // the extras items (only `target` is ever written)
    const uint32_t *drive_item; // [n_drives] drive (the caller's order) -> its item
    uint32_t n_drives;
};

// Is entry k of a retarget list one that xpbd_world_set_drive_targets accepts?  (`drive`: its index when it is.)  The rules of
// the host variant, on the device: in range, above its predecessor in the list, a finite target, an ANGLE target in [-pi, pi].
#if defined(__HIPCC__)
__device__ __forceinline__ bool drive_entry_valid(const DriveTable &t, const uint32_t *__restrict__ drives, const double *__restrict__ targets,
                                                  uint32_t k, uint32_t &drive)
{
    drive = drives ? drives[k] : k;
    if (drive >= t.n_drives || (drives && k && drives[k - 1] >= drive))
        return false;
    const double target = targets[k];
    if (!(target - target == 0.0)) // NaN, +-inf
        return false;
    const double pi = 3.14159265358979323846;
    return t.items[t.drive_item[drive]].kind != XPBD_DRIVE_ANGLE || (target >= -pi && target <= pi);
}
#endif

// One record per entry: joint joints[k] (NULL: joint k) into out[k]; an index >= t.n_joints gives kind = XPBD_JOINT_STATE_NO_JOINT
// and zeros.  out is 16-byte aligned.
hipError_t launch_joint_states(const BodyArrays &b, const JointStateTables &t, const uint32_t *joints, uint32_t n, xpbd_joint_state *out,
                               hipStream_t stream);
// items[drive_item[drives[k]]].target = targets[k] for every valid entry (drives == NULL: drive k).
hipError_t launch_drive_targets(const DriveTable &t, const uint32_t *drives, const double *targets, uint32_t n, hipStream_t stream);

} // namespace xpbd
