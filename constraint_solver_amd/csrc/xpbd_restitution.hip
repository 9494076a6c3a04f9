// xpbd_restitution.hip -- restitution for gfx950: the velocity pass after derive (include/xpbd.h, "RESTITUTION"), per substep,
// per body.  Split from xpbd_contacts.hip; declarations: xpbd_contacts.h.  What it shares with the other units of the
// pipeline: xpbd_contacts_device.hpp.
//
// Determinism: every floating-point sum is formed by ONE lane in a fixed order (neighbour index, then sweep, then manifold
// point index; the ground's vertices in vertex order); there are no atomics.  Both bodies of a pair run the same sequence on
// the same values, so results do not depend on launch order or on how the world is sharded.
#include "xpbd_contacts_device.hpp"

namespace xpbd {
namespace {

// What the pass needs of a body: pose and velocities after derive, velocities at the start of the substep, mass properties.
struct VelBody {
    Vec3 pos;
    Quat rot;
    Vec3 vel, ang, vel0, ang0;
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 com;
};

// post: the 13 dynamic fields after derive (SoA, as b.dyn); start: velocity and angular velocity at the start of the substep,
// [6][stride]
__device__ __forceinline__ VelBody load_vel_body(const double *__restrict__ post, const double *__restrict__ start, uint32_t st,
                                                 const ContactBuffers &c, uint32_t i)
{
    const BodyDynamic d = load_dynamic(post, st, i);
    const StatRecord s = load_stat_record(c.stat_rec, c.stat_index ? c.stat_index[i] : i);
    VelBody v;
    v.pos = d.pos, v.rot = d.rot, v.vel = d.vel, v.ang = d.ang;
    v.vel0 = load3(start, 0, st, i);
    v.ang0 = load3(start, 3, st, i);
    v.inv_mass = s.inv_mass;
    v.inv_inertia = s.inv_inertia;
    v.com = s.com;
    return v;
}

constexpr uint32_t kRestitutionSweeps = XPBD_RESTITUTION_SWEEPS; // passes over the points of one manifold

__device__ __forceinline__ double max_restitution(double a, double b) { return a < b ? b : a; }

// One lane per body.  Reads the post-derive state of every body from `post` and the start-of-substep velocities from `start`,
// writes the body's whole end-of-substep state to b.dyn, which no lane of this launch reads.
// TERRAIN: the ground part looks the terrain's plane up at every vertex of the mask again (the pose has moved since the
// integrate + ground stage): outside the field the vertex makes no entry, inside the plane's normal stands for (0, 0, 1).
template <bool TERRAIN>
__global__ void __launch_bounds__(kBlock) k_restitution(BodyArrays b, const double *__restrict__ post, const double *__restrict__ start,
                                                        ShapeTable shapes, ContactBuffers c, const uint32_t *__restrict__ ground_masks)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_integrate_ground
    uint32_t *lds_off = stage_shape_tables(lds, shapes);

    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t st = b.stride;
    VelBody self = load_vel_body(post, start, st, c, i);
    const double e_self = c.restitution[i], threshold = c.bounce_threshold;
    const Vec3 centre = self.pos + self.com;

    // pair contacts: Jacobi over the manifolds on the post-derive velocities, neighbour order
    Vec3 dv{0.0, 0.0, 0.0}, dw{0.0, 0.0, 0.0};
    uint32_t count = 0;
    const uint32_t k_end = c.nbr_off[i + 1];
    for (uint32_t k = c.nbr_off[i]; k < k_end; ++k) {
        const uint32_t pair = c.nbr_pair[k];
        const uint32_t code = c.pair_codes[pair];
        const uint32_t n_points = code & ((1u << kPairCodeFeatureShift) - 1u);
        if (!n_points)
            continue;
        const uint32_t j = c.nbr[k];
        const double e = max_restitution(e_self, c.restitution[j]); // (the larger of two values: the same from both sides)
        if (!(e > 0.0))
            continue;
        const VelBody other = load_vel_body(post, start, st, c, j);
        const Vec3 centre_other = other.pos + other.com;
        const ContactManifold *m = c.manifolds + pair;
        const uint32_t feature = code >> kPairCodeFeatureShift;
        // roles and points exactly as pair_solve_derive_body (xpbd_contacts.hip) forms them
        const bool self_is_a = i < j;
        const bool ref_is_a = feature != 1u;
        const bool self_is_inc = self_is_a != ref_is_a;
        const bool face = feature != 2u;
        const Plane ref_plane{Vec3{m->plane[0], m->plane[1], m->plane[2]}, m->plane[3]};
        // Sequential impulses inside the manifold, on copies of the two bodies' post-derive velocities: every point keeps the
        // impulse it has applied so far (never negative), kRestitutionSweeps passes in point order.  Both bodies of the pair
        // run the same sequence on the same values (3-vectors selected by role, w_inc + w_ref commutes): the same bits.
        Vec3 v_s = self.vel, w_s = self.ang, v_o = other.vel, w_o = other.ang;
        double total[kMaxManifoldPoints];
#pragma unroll
        for (uint32_t pt = 0; pt < kMaxManifoldPoints; ++pt)
            total[pt] = 0.0;
        uint32_t applied = 0;
        for (uint32_t sweep = 0; sweep < kRestitutionSweeps; ++sweep) {
#pragma unroll
            for (uint32_t pt = 0; pt < kMaxManifoldPoints; ++pt) { // (unrolled: total[] stays in registers)
                if (pt >= n_points)
                    break;
                const Vec3 p_inc{m->point[pt][0], m->point[pt][1], m->point[pt][2]};
                Vec3 p_ref, n;
                if (face) {
                    const double depth = distance(ref_plane, p_inc);
                    p_ref = p_inc - depth * ref_plane.normal;
                    n = ref_plane.normal;
                } else {
                    p_ref = Vec3{m->point[1][0], m->point[1][1], m->point[1][2]};
                    const Vec3 d = p_ref - p_inc;
                    const double len = length(d);
                    if (len == 0.0)
                        continue;
                    n = d * (1.0 / len);
                }
                const Vec3 p_self = self_is_inc ? p_inc : p_ref, p_other = self_is_inc ? p_ref : p_inc;
                const Vec3 arm = p_self - centre, arm_other = p_other - centre_other;
                const Vec3 u_self = v_s + cross(w_s, arm), u_other = v_o + cross(w_o, arm_other);
                const Vec3 u0_self = self.vel0 + cross(self.ang0, arm), u0_other = other.vel0 + cross(other.ang0, arm_other);
                const double vn = dot(n, self_is_inc ? u_self - u_other : u_other - u_self);      // incident - reference
                const double vn0 = dot(n, self_is_inc ? u0_self - u0_other : u0_other - u0_self);
                // w = w_incident + w_reference; IEEE addition commutes
                const double w = generalized_inverse_mass(self, p_self, n) + generalized_inverse_mass(other, p_other, n);
                if (!(vn0 < -threshold && w > 0.0))
                    continue;
                double wanted = total[pt] + ((-e) * vn0 - vn) / w;
                if (!(wanted > 0.0))
                    wanted = 0.0;
                const double lambda = wanted - total[pt];
                if (lambda == 0.0)
                    continue;
                total[pt] = wanted;
                const Vec3 plus = lambda * n, minus = (-lambda) * n; // on the incident, on the reference body
                const Vec3 impulse = self_is_inc ? plus : minus, impulse_other = self_is_inc ? minus : plus;
                v_s = v_s + impulse * self.inv_mass;
                w_s = w_s + cross(self.inv_inertia * arm, impulse);
                v_o = v_o + impulse_other * other.inv_mass;
                w_o = w_o + cross(other.inv_inertia * arm_other, impulse_other);
                ++applied;
            }
        }
        if (applied) { // one Jacobi entry per manifold that bounced
            dv = dv + (v_s - self.vel);
            dw = dw + (w_s - self.ang);
            ++count;
        }
    }
    if (count) {
        const double cnt = (double)count;
        self.vel = self.vel + dv / cnt;
        self.ang = self.ang + dw / cnt;
    }

    // ground: the vertices of this substep's contact mask in vertex order, each applied at once
    const double e_ground = max_restitution(e_self, c.ground_restitution);
    const uint32_t mask = ground_masks[i];
    if (e_ground > 0.0 && mask) {
        const uint32_t sid = b.shape_id[i];
        const double *verts = lds + 3 * lds_off[sid];
        const Frame frame{frame_origin(self.pos, self.rot, self.com), self.rot};
        Vec3 n{0.0, 0.0, 1.0};
        const double target_scale = -e_ground;
        for (uint32_t todo = mask; todo != 0; todo &= todo - 1) {
            const uint32_t v = __ffs(todo) - 1;
            const Vec3 p = frame * Vec3{verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
            if (TERRAIN) {
                Plane plane;
                if (!terrain_plane(c.terrain, p, plane))
                    continue;
                n = plane.normal;
            }
            const Vec3 arm = p - centre;
            const double vn = dot(n, self.vel + cross(self.ang, arm));
            const double vn0 = dot(n, self.vel0 + cross(self.ang0, arm));
            const double w = generalized_inverse_mass(self, p, n);
            const double target = target_scale * vn0;
            if (!(vn0 < -threshold && vn < target && w > 0.0))
                continue;
            const double lambda = (target - vn) / w;
            const Vec3 impulse = lambda * n;
            self.vel = self.vel + impulse * self.inv_mass;
            self.ang = self.ang + cross(self.inv_inertia * arm, impulse);
        }
    }

    BodyDynamic d;
    d.pos = self.pos, d.rot = self.rot, d.vel = self.vel, d.ang = self.ang;
    store_dynamic(b.dyn, st, i, d);
}

// The pass has no subset form.  The bodies a BodySubset skips (the sleepers of a world with sleeping on) are put back
// afterwards from `post`, which holds their state as it was: one lane per body, 13 stores for a skipped one.
__global__ void __launch_bounds__(kBlock) k_restitution_put_back(BodyArrays b, const double *__restrict__ post, const uint8_t *__restrict__ skip)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n || !skip[i])
        return;
    for (uint32_t f = 0; f < kDynFields; ++f)
        b.dyn[(size_t)f * b.stride + i] = post[(size_t)f * b.stride + i];
}

} // namespace

hipError_t launch_restitution(const BodyArrays &b, const double *post, const double *start, const ShapeTable &s, const ContactBuffers &c,
                              const uint32_t *ground_masks, hipStream_t stream, const BodySubset &subset)
{
    if (b.n == 0)
        return hipSuccess;
    if (!c.restitution || post == b.dyn || start == b.dyn || subset.list)
        return hipErrorInvalidValue; // (the kernel writes b.dyn while other lanes read `post` and `start`; it has no list form)
    const size_t lds_bytes = shape_lds_bytes(s);
    if (c.terrain.planes)
        hipLaunchKernelGGL(k_restitution<true>, dim3(blocks_for(b.n)), dim3(kBlock), lds_bytes, stream, b, post, start, s, c, ground_masks);
    else
        hipLaunchKernelGGL(k_restitution<false>, dim3(blocks_for(b.n)), dim3(kBlock), lds_bytes, stream, b, post, start, s, c, ground_masks);
    if (subset.skip)
        hipLaunchKernelGGL(k_restitution_put_back, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, post, subset.skip);
    return hipGetLastError();
}

} // namespace xpbd
