// xpbd_damping.hip -- DAMPING (EXTENSION) for gfx950: stage 7 of a substep, the velocity pass after restitution
// (include/xpbd.h, "DAMPING"); declarations: xpbd_damping.h.
//
// k_body_damping is one lane per body, in place on the six velocity fields of the SoA state: six coalesced 8-byte loads, the
// body's four row fields (SoA as well), drag, caps, six stores -- 128 bytes a body beside the mass record that tells a FIXED
// body.  k_joint_damping, launched only when a joint has a damper, is one lane per body walking the body's joints through the
// CSR of xpbd_world_set_joints: a gather of the joint record, of its (mu_l, mu_a) and of the other end's state, the Jacobi sum
// in joint order by that one lane, and six stores to a scratch that k_body_damping then takes the velocities from (other
// lanes still read the stage-6 velocities of the SoA state).  No LDS, no atomics, no scratch memory.
//
// Determinism: every sum is formed by ONE lane in a fixed order; both ends of a joint evaluate the same expressions on the same
// values (3-vectors selected by role), so results do not depend on launch order.  Built without contraction, as every unit.
#include "xpbd_contacts_device.hpp"
#include "xpbd_damping.h"

namespace xpbd {
namespace {

// What the kernels need of the world beside the bodies and the damping tables (a handful of pointers, not ContactBuffers).
struct DampingWorld {
    const double *stat_rec;
    const uint32_t *stat_index;
    const Joint *joints;
    const uint32_t *joint_off, *joint_list;
    const uint8_t *skip;
};

// Does stage 7 work on body i?  Awake, and not FIXED: inverse_mass and all nine inverse_inertia entries == 0 (`s`: its record).
__device__ __forceinline__ bool damped_body(const DampingWorld &w, uint32_t i, StatRecord &s)
{
    if (w.skip && w.skip[i])
        return false;
    s = load_stat_record(w.stat_rec, w.stat_index ? w.stat_index[i] : i);
    const Mat3 &m = s.inv_inertia;
    const bool fixed = s.inv_mass == 0.0 && m.cx.x == 0.0 && m.cx.y == 0.0 && m.cx.z == 0.0 && m.cy.x == 0.0 && m.cy.y == 0.0 && m.cy.z == 0.0 &&
                       m.cz.x == 0.0 && m.cz.y == 0.0 && m.cz.z == 0.0;
    return !fixed;
}

// One end of a joint as stage 6 left it (the fields generalized_inverse_mass reads, and the velocities).
struct DampBody {
    Vec3 pos;
    Quat rot;
    Vec3 vel, ang;
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 com;
};

__device__ __forceinline__ DampBody make_damp_body(const BodyDynamic &d, const StatRecord &s)
{
    DampBody o;
    o.pos = d.pos, o.rot = d.rot, o.vel = d.vel, o.ang = d.ang;
    o.inv_mass = s.inv_mass;
    o.inv_inertia = s.inv_inertia;
    o.com = s.com;
    return o;
}

// k of a damper: the share of the relative velocity a substep removes, at most all of it.
__device__ __forceinline__ double damper_share(double mu, double h) { return mu * h < 1.0 ? mu * h : 1.0; }

// The joint part: reads the stage-6 state of every body from b.dyn, writes the two velocities of the bodies it works on to
// t.scratch ([6][stride]).  A body without an entry gets its velocities unchanged.
__global__ void __launch_bounds__(kBlock) k_joint_damping(BodyArrays b, DampingTables t, double h, DampingWorld w)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    StatRecord stat;
    if (!damped_body(w, i, stat))
        return;
    const uint32_t st = b.stride;
    const DampBody self = make_damp_body(load_dynamic(b.dyn, st, i), stat);

    Vec3 dv{0.0, 0.0, 0.0}, dw{0.0, 0.0, 0.0};
    uint32_t count = 0;
    const uint32_t k_end = w.joint_off[i + 1];
    for (uint32_t k = w.joint_off[i]; k < k_end; ++k) { // ascending joint index
        const uint32_t joint = w.joint_list[k];
        const double2 mu = t.joint_mu[joint];
        if (!(mu.x > 0.0) && !(mu.y > 0.0))
            continue;
        const Joint &jt = w.joints[joint];
        const bool self_is_a = jt.body_a == i;
        const uint32_t j = self_is_a ? jt.body_b : jt.body_a;
        const DampBody other = make_damp_body(load_dynamic(b.dyn, st, j), load_stat_record(w.stat_rec, w.stat_index ? w.stat_index[j] : j));
        // evaluated per body, 3-vectors selected by role (a / b) as in the position pass: both ends form the same values (IEEE
        // addition commutes), each keeps the changes of its own end
        Vec3 e_dv{0.0, 0.0, 0.0}, e_dw{0.0, 0.0, 0.0};
        uint32_t terms = 0;
        if (mu.x > 0.0) { // linear: the relative velocity of the two anchors
            const Vec3 anchor_self = self_is_a ? Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]} : Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]};
            const Vec3 anchor_other = self_is_a ? Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]} : Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]};
            const Vec3 p_self = Frame{frame_origin(self.pos, self.rot, self.com), self.rot} * anchor_self;
            const Vec3 p_other = Frame{frame_origin(other.pos, other.rot, other.com), other.rot} * anchor_other;
            const Vec3 arm = p_self - (self.pos + self.com), arm_other = p_other - (other.pos + other.com);
            const Vec3 u_self = self.vel + cross(self.ang, arm), u_other = other.vel + cross(other.ang, arm_other);
            const Vec3 d = self_is_a ? u_other - u_self : u_self - u_other; // u_b(p_b) - u_a(p_a)
            const double len = length(d);
            if (len != 0.0) {
                const Vec3 n = d * (1.0 / len);
                const double w_s = generalized_inverse_mass(self, p_self, n), w_o = generalized_inverse_mass(other, p_other, n);
                const double w_sum = self_is_a ? w_s + w_o : w_o + w_s; // W_a + W_b
                if (w_sum > 0.0) {
                    const double lambda = (damper_share(mu.x, h) * len) / w_sum;
                    const Vec3 impulse = self_is_a ? lambda * n : (-lambda) * n;
                    e_dv = e_dv + impulse * self.inv_mass;
                    e_dw = e_dw + cross(self.inv_inertia * arm, impulse);
                    ++terms;
                }
            }
        }
        if (mu.y > 0.0) { // angular: the relative angular velocity, on the same stage-6 values
            const Vec3 d = self_is_a ? other.ang - self.ang : self.ang - other.ang; // w_b - w_a
            const double len = length(d);
            if (len != 0.0) {
                const Vec3 n = d * (1.0 / len);
                const Vec3 n_self = conjugate(self.rot) * n, n_other = conjugate(other.rot) * n;
                const double w_s = dot(self.inv_inertia * n_self, n_self), w_o = dot(other.inv_inertia * n_other, n_other);
                const double w_ang = self_is_a ? w_s + w_o : w_o + w_s; // the angular w of the limits
                if (w_ang > 0.0) {
                    const double lambda = (damper_share(mu.y, h) * len) / w_ang;
                    const Vec3 turn = self_is_a ? lambda * n : (-lambda) * n;
                    e_dw = e_dw + self.rot * (self.inv_inertia * (conjugate(self.rot) * turn));
                    ++terms;
                }
            }
        }
        if (terms) { // one Jacobi entry per joint that damped
            dv = dv + e_dv;
            dw = dw + e_dw;
            ++count;
        }
    }
    Vec3 vel = self.vel, ang = self.ang;
    if (count) {
        const double cnt = (double)count;
        vel = vel + dv / cnt;
        ang = ang + dw / cnt;
    }
    store3(t.scratch, 0, st, i, vel);
    store3(t.scratch, 3, st, i, ang);
}

// v * s, then the cap: what steps 2 and 3 do to one of the two velocities.
__device__ __forceinline__ Vec3 drag_and_cap(Vec3 v, double h, double drag, double cap)
{
    const double s = 1.0 / (1.0 + h * drag);
    v = v * s;
    const double m = length(v);
    if (m > cap)
        v = v * (cap / m);
    return v;
}

// Drag and caps: the velocities come from vel_in ([6][stride]: the joint part's scratch, or fields D_VEL.. of b.dyn themselves;
// a lane reads and writes its own body only) and go to b.dyn.
__global__ void __launch_bounds__(kBlock) k_body_damping(BodyArrays b, DampingTables t, const double *vel_in, double h, DampingWorld w)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    StatRecord stat;
    if (!damped_body(w, i, stat))
        return;
    const uint32_t st = b.stride;
    double row[kDampingRowFields] = {0.0, 0.0, __builtin_inf(), __builtin_inf()};
    if (t.rows) {
#pragma unroll
        for (uint32_t f = 0; f < kDampingRowFields; ++f)
            row[f] = t.rows[(size_t)f * t.row_stride + i];
    }
    const Vec3 vel = drag_and_cap(load3(vel_in, 0, st, i), h, row[0], row[2]);
    const Vec3 ang = drag_and_cap(load3(vel_in, 3, st, i), h, row[1], row[3]);
    store3(b.dyn, D_VEL, st, i, vel);
    store3(b.dyn, D_ANG, st, i, ang);
}

} // namespace

hipError_t launch_damping(const BodyArrays &b, const DampingTables &t, double h, const ContactBuffers &c, hipStream_t stream, const BodySubset &subset)
{
    static_assert(D_ANG == D_VEL + 3, "the two velocities are one block of six fields");
    if (b.n == 0 || (!t.rows && !t.joint_mu))
        return hipSuccess;
    if (subset.list || !c.stat_rec || (t.joint_mu && (!t.scratch || !c.joint_off)))
        return hipErrorInvalidValue;
    const DampingWorld w{c.stat_rec, c.stat_index, c.joints, c.joint_off, c.joint_list, subset.skip};
    const double *vel_in = b.dyn + (size_t)D_VEL * b.stride;
    if (t.joint_mu) {
        hipLaunchKernelGGL(k_joint_damping, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, t, h, w);
        vel_in = t.scratch;
    }
    hipLaunchKernelGGL(k_body_damping, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, t, vel_in, h, w);
    return hipGetLastError();
}

} // namespace xpbd
