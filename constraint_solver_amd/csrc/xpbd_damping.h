// xpbd_damping.h -- DAMPING (EXTENSION): the tables and the launcher of xpbd_damping.hip.  Semantics: include/xpbd.h, "DAMPING".
#pragma once

#include "xpbd_contacts.h"

namespace xpbd {

constexpr uint32_t kDampingRowFields = 4; // linear, angular, max_linear_speed, max_angular_speed

// What stage 7 reads beside the bodies and the joints of ContactBuffers.
struct DampingTables {
    // The body rows, SoA: field f of body i at rows[f * row_stride + i] (consecutive lanes read consecutive doubles, and a
    // population change gathers every field with the per-table gather of doubles).  NULL: every body has the default row.
    const double *rows;
    uint32_t row_stride;
    // (mu_l, mu_a) of every joint of ContactBuffers::joints, 16 bytes each.  NULL: no joint has a damper.
    const double2 *joint_mu;
    // [6][stride], the layout of fields D_VEL.. of the SoA state: where the joint part leaves the velocities of the bodies it
    // works on, because other lanes still read the stage-6 velocities of b.dyn.  Only read and written with joint_mu.
    double *scratch;
};

// Stage 7 of a substep on b.dyn, which holds every body's end-of-substep state: with t.joint_mu one launch of the joint part
// (every body it works on -> t.scratch), then one launch of k_body_damping, which applies drag and caps to the velocities it
// takes from t.scratch or, without joint dampers, from b.dyn itself, and writes them to b.dyn.  The bodies subset.skip marks and
// the FIXED ones are left alone by both.  (No list form.)
hipError_t launch_damping(const BodyArrays &b, const DampingTables &t, double h, const ContactBuffers &c, hipStream_t stream,
                          const BodySubset &subset = BodySubset());

} // namespace xpbd
