// xpbd_kinematic.h -- KINEMATIC bodies (EXTENSION): launchers for xpbd_kinematic.hip.  Semantics: include/xpbd.h, "KINEMATIC
// bodies".  The table is the caller's xpbd_kinematic list on the device, ascending by body; k_kinematic_velocities overwrites
// the two velocities of every entry's body before an integrate stage, k_kinematic_retarget writes the seven value doubles of
// resident entries, k_kinematic_mass gathers what xpbd_world_set_kinematics checks.
#pragma once

#include "xpbd_kernels.h"

namespace xpbd {

// The kinematic table of a world as the kernels read it (only linear / angular are ever written).
struct KinematicTable {
    xpbd_kinematic *entries;
    uint32_t n;
};

constexpr uint32_t kKinematicRowDoubles = 7;  // linear[3], angular[4]
constexpr uint32_t kKinematicMassDoubles = 10; // inverse_mass, inverse_inertia[9]

// Is entry k of a retarget list one that xpbd_world_set_kinematic_targets accepts?  (`entry`: its index when it is.)  The rules
// of the host variant, on the device: in range, above its predecessor in the list, seven finite values, a POSE rotation that
// is not all zero.
#if defined(__HIPCC__)
__device__ __forceinline__ bool kinematic_entry_valid(const KinematicTable &t, const uint32_t *__restrict__ entries, const double *__restrict__ rows,
                                                      uint32_t k, uint32_t &entry)
{
    entry = entries ? entries[k] : k;
    if (entry >= t.n || (entries && k && entries[k - 1] >= entry))
        return false;
    const double *row = rows + (size_t)k * kKinematicRowDoubles;
    bool finite = true;
#pragma unroll
    for (uint32_t c = 0; c < kKinematicRowDoubles; ++c)
        finite = finite && (row[c] - row[c] == 0.0); // NaN, +-inf
    if (!finite)
        return false;
    return t.entries[entry].mode != XPBD_KINEMATIC_POSE || row[3] != 0.0 || row[4] != 0.0 || row[5] != 0.0 || row[6] != 0.0;
}
#endif

// The overwrite before the integrate stage of a substep with `left` (>= 1) substeps of h to go, this one included.  moving
// (NULL: not wanted; [b.stride], zeroed by the caller): moving[body] = 1 for every entry whose body is MOVING ("SLEEPING").
hipError_t launch_kinematic_velocities(const BodyArrays &b, const KinematicTable &t, double h, uint32_t left, uint8_t *moving, hipStream_t stream);
// entries[entries[k]].linear / .angular = rows[k] for every valid entry (entries == NULL: entry k).
hipError_t launch_kinematic_retarget(const KinematicTable &t, const uint32_t *entries, const double *rows, uint32_t n, hipStream_t stream);
// out[k][0..9] = inverse_mass and inverse_inertia of body t.entries[k].body (zeros for a body outside the world).
hipError_t launch_kinematic_mass(const BodyArrays &b, const KinematicTable &t, double *out, hipStream_t stream);

} // namespace xpbd
