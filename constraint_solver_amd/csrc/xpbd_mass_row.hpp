// xpbd_mass_row.hpp -- one row of a MASS edit (include/xpbd.h, "MASS properties of resident bodies"): the value rules and the
// DIRECT inversion, the same code for the host variant's argument check (xpbd_checks.cpp) and for the lanes of k_set_mass
// (xpbd_mass_edit.hip), as kinematic_entry_valid shares the rules of a retarget.  No HIP header: builds with plain g++.  Every
// unit that includes it is built without contraction, so host and device form the same determinant, bit for bit.
#pragma once

#include <cstdint>

#include "../../include/xpbd.h"
#include "xpbd_math.hpp"

#if defined(__HIPCC__)
#define XPBD_MASS_UNROLL _Pragma("unroll")
#else
#define XPBD_MASS_UNROLL
#endif

namespace xpbd {

constexpr uint32_t kMassRowDoubles = 13;   // inverse_mass | mass, inverse_inertia[9] | inertia[9], center_of_mass[3]
constexpr uint32_t kMassFixedDoubles = 10; // what makes a body fixed: inverse_mass and inverse_inertia[9] all == 0
constexpr uint32_t kMassLayoutBits = 0xFFu; // flags & kMassLayoutBits is the layout, the bits above are XPBD_MASS_KEEP_FRAME or unknown

enum MassRowVerdict : uint32_t {
    kMassRowOk = 0,
    kMassRowNotFinite,           // a NaN or an infinity among the 13 values
    kMassRowNegativeInverseMass, // INVERSE: inverse_mass < 0
    kMassRowMassNotPositive,     // DIRECT: mass <= 0
    kMassRowSingular             // DIRECT: the determinant of the tensor == 0 (Rigid::new panics)
};

// Unknown flag bits, or a layout other than XPBD_MASS_INVERSE / XPBD_MASS_DIRECT?
XPBD_HD bool mass_flags_known(uint32_t flags)
{
    return (flags & ~(kMassLayoutBits | XPBD_MASS_KEEP_FRAME)) == 0u && (flags & kMassLayoutBits) <= XPBD_MASS_DIRECT;
}

// `row` as the caller wrote it -> `out`, the 13 doubles the body takes (INVERSE layout).  DIRECT is Rigid::new (src/rigid.rs:53-71):
// 1.0 / mass and cgmath's Matrix3::invert, determinant first.  `out` is written only with kMassRowOk.
XPBD_HD MassRowVerdict resolve_mass_row(const double *row, uint32_t layout, double *out)
{
    bool finite = true;
    XPBD_MASS_UNROLL
    for (uint32_t c = 0; c < kMassRowDoubles; ++c)
        finite = finite && (row[c] - row[c] == 0.0); // NaN, +-inf
    if (!finite)
        return kMassRowNotFinite;
    if (layout != XPBD_MASS_DIRECT) {
        if (row[0] < 0.0)
            return kMassRowNegativeInverseMass;
        XPBD_MASS_UNROLL
        for (uint32_t c = 0; c < kMassRowDoubles; ++c)
            out[c] = row[c];
        return kMassRowOk;
    }
    if (!(row[0] > 0.0))
        return kMassRowMassNotPositive;
    const Mat3 tensor{Vec3{row[1], row[2], row[3]}, Vec3{row[4], row[5], row[6]}, Vec3{row[7], row[8], row[9]}};
    Mat3 inv;
    if (!invert(tensor, inv))
        return kMassRowSingular;
    out[0] = 1.0 / row[0];
    out[1] = inv.cx.x, out[2] = inv.cx.y, out[3] = inv.cx.z;
    out[4] = inv.cy.x, out[5] = inv.cy.y, out[6] = inv.cy.z;
    out[7] = inv.cz.x, out[8] = inv.cz.y, out[9] = inv.cz.z;
    out[10] = row[10], out[11] = row[11], out[12] = row[12];
    return kMassRowOk;
}

// Do the 13 doubles a body takes leave it FIXED (the islands' definition)?  The kinematic rule: a body with an entry in the
// kinematic table takes no other row.
XPBD_HD bool mass_row_fixed(const double *out)
{
    bool fixed = true;
    XPBD_MASS_UNROLL
    for (uint32_t c = 0; c < kMassFixedDoubles; ++c)
        fixed = fixed && out[c] == 0.0;
    return fixed;
}

} // namespace xpbd
