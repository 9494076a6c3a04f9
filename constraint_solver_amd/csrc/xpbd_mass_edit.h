// xpbd_mass_edit.h -- MASS properties of resident bodies (EXTENSION): launchers for xpbd_mass_edit.hip.  Semantics: include/xpbd.h,
// "MASS properties of resident bodies"; the value rules of a row: xpbd_mass_row.hpp.  k_set_mass writes the 13 mass doubles of
// the listed bodies (and, with XPBD_MASS_KEEP_FRAME, their position and velocity), k_get_mass gathers them.
#pragma once

#include "xpbd_kernels.h"
#include "xpbd_kinematic.h"
#include "xpbd_mass_row.hpp"

namespace xpbd {

// One call's list, all device pointers: entry k names body indices[k] (NULL: body k) and carries rows[13k..13k+12].
// owner ([b.stride] words, or NULL): where the list may name a body twice (the device variant), the valid entries first claim
// their body there and only the entry that holds the claim is applied -- one entry wins whole.  NULL: the caller has seen the
// indices and they are distinct.
struct MassEditList {
    const uint32_t *indices;
    const double *rows;
    uint32_t n;
    uint32_t flags; // XPBD_MASS_* (known bits only: the caller has checked them)
    uint32_t *owner;
};

// An entry is SKIPPED (it changes nothing) when its index is outside the world, resolve_mass_row refuses its row, or its body has
// an entry in `kinematic` (ascending by body) and the row would not leave it fixed.  More than kMaxEditEntries (2^29) entries or
// rows that are not 8-byte aligned: hipErrorInvalidValue.
hipError_t launch_set_mass(const BodyArrays &b, const KinematicTable &kinematic, const MassEditList &list, hipStream_t stream);
// rows[13k..13k+12] = inverse_mass, inverse_inertia[9], center_of_mass[3] of body indices[k] (NULL: body k); zeros for an index
// outside the world.
hipError_t launch_get_mass(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *rows, hipStream_t stream);

} // namespace xpbd
