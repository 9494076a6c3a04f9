// xpbd_joint_state.hip -- joint STATES and drive TARGETS (EXTENSION) for gfx950.  Semantics: include/xpbd.h, "Joint STATES and
// drive TARGETS"; the tables: xpbd_joint_state.h.
//
// k_joint_states is one lane per requested joint: a gather of the joint record (128 bytes), of the two bodies' pose, velocity
// and centre of mass from the SoA arrays (19 doubles each), of the joint's rows of the angular-limit CSR and of its extras
// items, and five 16-byte stores.  No shared memory, no atomics.  Every quantity is the expression joint_limit_terms,
// pair_solve_derive_body and k_joint_extras (xpbd_contacts.hip) evaluate, operand for operand, so that a limit reported as
// violated is one the next substep acts on at these poses; the unit is built without contraction, as they are.
// k_drive_targets is one lane per entry of a retarget list and writes one double.
#include <hip/hip_runtime.h>

#include "xpbd_device.hpp"
#include "xpbd_joint_state.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

// What the states read of one end of a joint.
struct StateBody {
    Vec3 pos, vel, ang, com;
    Quat rot;
};

__device__ __forceinline__ StateBody load_state_body(const BodyArrays &b, uint32_t i)
{
    StateBody s;
    s.pos = load3(b.dyn, D_POS, b.stride, i);
    s.rot = load_quat(b.dyn, D_ROT, b.stride, i);
    s.vel = load3(b.dyn, D_VEL, b.stride, i);
    s.ang = load3(b.dyn, D_ANG, b.stride, i);
    s.com = load3(b.stat, S_COM, b.stride, i);
    return s;
}

__device__ __forceinline__ Vec3 vec3_of(const double *v) { return Vec3{v[0], v[1], v[2]}; }

// phi of XPBD_LIMIT_HINGE and of the angular drives: the signed angle about a_w from r_a to r_b.
__device__ __forceinline__ double hinge_phi(Quat q_a, Quat q_b, const double *ref_a, const double *ref_b, Vec3 a_w)
{
    const Vec3 r_a = q_a * vec3_of(ref_a), r_b = q_b * vec3_of(ref_b);
    return atan2(dot(cross(r_a, r_b), a_w), dot(r_a, r_b));
}

__device__ __forceinline__ void store_state(xpbd_joint_state *out, const double v[8], uint32_t joint, uint32_t kind, uint32_t flags)
{
    double2 *o = reinterpret_cast<double2 *>(out);
    o[0] = double2{v[0], v[1]};
    o[1] = double2{v[2], v[3]};
    o[2] = double2{v[4], v[5]};
    o[3] = double2{v[6], v[7]};
    reinterpret_cast<uint4 *>(out)[4] = uint4{joint, kind, flags, 0u};
}

__global__ void __launch_bounds__(kBlock) k_joint_states(BodyArrays b, JointStateTables t, const uint32_t *__restrict__ joints, uint32_t n,
                                                         xpbd_joint_state *__restrict__ out)
{
    static_assert(sizeof(xpbd_joint_state) == 80 && offsetof(xpbd_joint_state, joint) == 64, "five 16-byte stores");
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t joint = joints ? joints[k] : k;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // separation, misalignment, angle, angle_rate, travel, travel_rate, swing, twist
    if (joint >= t.n_joints) {
        store_state(out + k, v, 0u, XPBD_JOINT_STATE_NO_JOINT, 0u);
        return;
    }
    const Joint &jt = t.joints[joint];
    if (jt.body_a >= b.n || jt.body_b >= b.n) { // (never: the setters refuse such a joint)
        store_state(out + k, v, 0u, XPBD_JOINT_STATE_NO_JOINT, 0u);
        return;
    }
    const StateBody a = load_state_body(b, jt.body_a), bb = load_state_body(b, jt.body_b);
    uint32_t flags = 0;
    const Vec3 p_a = Frame{frame_origin(a.pos, a.rot, a.com), a.rot} * vec3_of(jt.anchor_a);
    const Vec3 p_b = Frame{frame_origin(bb.pos, bb.rot, bb.com), bb.rot} * vec3_of(jt.anchor_b);
    const Vec3 d = p_b - p_a;
    const Vec3 a_w = a.rot * vec3_of(jt.axis_a);
    const Vec3 b_w = bb.rot * vec3_of(jt.axis_b);
    const double s = dot(d, a_w);

    if (jt.kind == XPBD_JOINT_SLIDER) {
        v[0] = length(d - a_w * s); // the perpendicular term's len
        v[4] = s;
        // d/dt (d . a_w) with a_w carried by body a
        const Vec3 v_pa = a.vel + cross(a.ang, p_a - (a.pos + a.com)), v_pb = bb.vel + cross(bb.ang, p_b - (bb.pos + bb.com));
        v[5] = dot(v_pb - v_pa, a_w) + dot(d, cross(a.ang, a_w));
        flags |= XPBD_JOINT_STATE_HAS_TRAVEL;
    } else {
        v[0] = length(d) - jt.distance; // the positional term's error
    }
    if (jt.kind != XPBD_JOINT_DISTANCE)
        v[1] = length(cross(a_w, b_w)); // the angular term's mag

    // the joint's extras: its SLIDE limit and its angular drive
    const double *ref_a = nullptr, *ref_b = nullptr;
    const uint32_t slot = t.extra_slot ? t.extra_slot[joint] : kNoExtraSlot;
    if (slot != kNoExtraSlot) {
        const uint32_t e_end = t.extra_off[slot + 1];
        for (uint32_t e = t.extra_off[slot]; e < e_end; ++e) {
            const JointExtraItem &it = t.extra_items[e];
            if (it.kind == kExtraSlideLimit) { // target = lower, compliance = upper
                flags |= s < it.target ? XPBD_JOINT_STATE_TRAVEL_BELOW : (s > it.compliance ? XPBD_JOINT_STATE_TRAVEL_ABOVE : 0u);
            } else if (it.kind == XPBD_DRIVE_ANGLE || it.kind == XPBD_DRIVE_ANGULAR_VELOCITY) {
                ref_a = it.ref_a;
                ref_b = it.ref_b;
                flags |= XPBD_JOINT_STATE_ANGLE_OF_DRIVE;
            }
        }
    }
    // its angular limits, each with its own references
    bool swing_wanted = false;
    if (t.limit_off) {
        const uint32_t l_end = t.limit_off[joint + 1];
        for (uint32_t l = t.limit_off[joint]; l < l_end; ++l) {
            const JointLimit &lim = t.limits[l];
            if (lim.kind == XPBD_LIMIT_HINGE) {
                const double phi = hinge_phi(a.rot, bb.rot, lim.ref_a, lim.ref_b, a_w);
                flags |= phi < lim.lower ? XPBD_JOINT_STATE_ANGLE_BELOW : (phi > lim.upper ? XPBD_JOINT_STATE_ANGLE_ABOVE : 0u);
                if (!ref_a) {
                    ref_a = lim.ref_a;
                    ref_b = lim.ref_b;
                }
            } else if (lim.kind == XPBD_LIMIT_SWING) {
                swing_wanted = true;
                const Vec3 cr = cross(a_w, b_w);
                const double len = length(cr);
                if (len != 0.0 && atan2(len, dot(a_w, b_w)) > lim.upper)
                    flags |= XPBD_JOINT_STATE_SWING_ABOVE;
            } else { // XPBD_LIMIT_TWIST
                swing_wanted = true;
                const Vec3 bisector = a_w + b_w;
                const double len = length(bisector);
                if (len != 0.0) {
                    const Vec3 nrm = bisector * (1.0 / len);
                    Vec3 q_a = a.rot * vec3_of(lim.ref_a), q_b = bb.rot * vec3_of(lim.ref_b);
                    q_a = q_a - nrm * dot(q_a, nrm);
                    q_b = q_b - nrm * dot(q_b, nrm);
                    const double phi = atan2(dot(cross(q_a, q_b), nrm), dot(q_a, q_b));
                    v[7] = phi;
                    flags |= XPBD_JOINT_STATE_HAS_TWIST | (phi < lim.lower ? XPBD_JOINT_STATE_TWIST_BELOW : (phi > lim.upper ? XPBD_JOINT_STATE_TWIST_ABOVE : 0u));
                }
            }
        }
    }
    if (swing_wanted) {
        v[6] = atan2(length(cross(a_w, b_w)), dot(a_w, b_w));
        flags |= XPBD_JOINT_STATE_HAS_SWING;
    }
    if (ref_a) {
        v[2] = hinge_phi(a.rot, bb.rot, ref_a, ref_b, a_w);
        v[3] = dot(bb.ang - a.ang, a_w);
        flags |= XPBD_JOINT_STATE_HAS_ANGLE;
    }
    store_state(out + k, v, joint, jt.kind, flags);
}

__global__ void __launch_bounds__(kBlock) k_drive_targets(DriveTable t, const uint32_t *__restrict__ drives, const double *__restrict__ targets, uint32_t n)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    uint32_t drive;
    if (drive_entry_valid(t, drives, targets, k, drive))
        t.items[t.drive_item[drive]].target = targets[k];
}

} // namespace

hipError_t launch_joint_states(const BodyArrays &b, const JointStateTables &t, const uint32_t *joints, uint32_t n, xpbd_joint_state *out,
                               hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_joint_states, dim3(blocks_of(n)), dim3(kBlock), 0, stream, b, t, joints, n, out);
    return hipGetLastError();
}

hipError_t launch_drive_targets(const DriveTable &t, const uint32_t *drives, const double *targets, uint32_t n, hipStream_t stream)
{
    if (n == 0 || t.n_drives == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_drive_targets, dim3(blocks_of(n)), dim3(kBlock), 0, stream, t, drives, targets, n);
    return hipGetLastError();
}

} // namespace xpbd
