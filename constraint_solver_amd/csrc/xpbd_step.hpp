// xpbd_step.hpp -- the per-body substep of solver::step (reference src/solver.rs:6-16) as device
// functions, shared by the fused stepper (xpbd_kernels.hip) and the contact pipeline
// (xpbd_contacts.hip; the terrain lookup also xpbd_restitution.hip and xpbd_terrain.hip).  All arithmetic keeps the
// reference's operation order.  Where a square root is followed by the reciprocal of its own result (the three places
// of a substep that normalize), both correctly rounded values come from one sequence of xpbd_exact.hpp: the same bits as
// `sqrt` and `1.0 / s` in fewer f64 issue slots.  (The quotients by h of derive_body stay plain: DESIGN section 4.)
#pragma once

#include "xpbd_device.hpp"
#include "xpbd_exact.hpp"

namespace xpbd {

// normalized(Quat) of xpbd_math.hpp, |q| and 1 / |q| from one sequence.
__device__ __forceinline__ Quat normalized_exact(Quat q)
{
    const double m2 = q.s * q.s + (q.x * q.x + q.y * q.y + q.z * q.z);
    double m, k;
    exact::sqrt_and_reciprocal(m2, m, k);
    return Quat{q.s * k, q.x * k, q.y * k, q.z * k};
}

// Per-body state held in registers.
struct BodyStatic {
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 ext_force, int_force, ext_torque, int_torque;
    Vec3 com;
};

struct BodyDynamic {
    Vec3 pos;
    Quat rot;
    Vec3 vel;
    Vec3 ang;
};

__device__ __forceinline__ BodyStatic load_static(const BodyArrays &b, uint32_t i)
{
    const uint32_t st = b.stride;
    BodyStatic s;
    s.inv_mass = b.stat[(size_t)S_INV_MASS * st + i];
    s.inv_inertia.cx = load3(b.stat, S_INV_INERTIA + 0, st, i);
    s.inv_inertia.cy = load3(b.stat, S_INV_INERTIA + 3, st, i);
    s.inv_inertia.cz = load3(b.stat, S_INV_INERTIA + 6, st, i);
    s.ext_force = load3(b.stat, S_EXT_FORCE, st, i);
    s.int_force = load3(b.stat, S_INT_FORCE, st, i);
    s.ext_torque = load3(b.stat, S_EXT_TORQUE, st, i);
    s.int_torque = load3(b.stat, S_INT_TORQUE, st, i);
    s.com = load3(b.stat, S_COM, st, i);
    return s;
}

__device__ __forceinline__ BodyDynamic load_dynamic(const double *dyn, uint32_t st, uint32_t i)
{
    BodyDynamic d;
    d.pos = load3(dyn, D_POS, st, i);
    d.rot = load_quat(dyn, D_ROT, st, i);
    d.vel = load3(dyn, D_VEL, st, i);
    d.ang = load3(dyn, D_ANG, st, i);
    return d;
}

__device__ __forceinline__ void store_quat(double *base, uint32_t field, uint32_t st, uint32_t i, Quat q)
{
    base[(size_t)(field + 0) * st + i] = q.s;
    base[(size_t)(field + 1) * st + i] = q.x;
    base[(size_t)(field + 2) * st + i] = q.y;
    base[(size_t)(field + 3) * st + i] = q.z;
}

__device__ __forceinline__ void store_dynamic(double *dyn, uint32_t st, uint32_t i, const BodyDynamic &d)
{
    store3(dyn, D_POS, st, i, d.pos);
    store_quat(dyn, D_ROT, st, i, d.rot);
    store3(dyn, D_VEL, st, i, d.vel);
    store3(dyn, D_ANG, st, i, d.ang);
}

// What one substep keeps from before/after the integration.
struct SubstepFrames {
    Vec3 past_pos;  // src/solver.rs:7
    Quat past_rot;  // src/solver.rs:8
    Frame past;     // src/solver.rs:9  rigid.frame() before integrate
    Frame cur;      // rigid.frame() after integrate: frozen for the whole of ground() (src/collision.rs:17,24)
};

// src/solver.rs:7-10: remember the past pose, then Rigid::integrate (src/rigid.rs:82-99).
__device__ __forceinline__ SubstepFrames integrate_body(BodyDynamic &d, const BodyStatic &s, double h)
{
    SubstepFrames f;
    f.past_pos = d.pos;
    f.past_rot = d.rot;
    f.past = Frame{frame_origin(d.pos, d.rot, s.com), d.rot};

    const Vec3 force = s.ext_force + d.rot * s.int_force;
    d.vel = d.vel + (h * force) * s.inv_mass;
    d.pos = d.pos + h * d.vel;

    const Vec3 torque = s.ext_torque + d.rot * s.int_torque;
    d.ang = d.ang + (h * s.inv_inertia) * torque;
    const Quat dq = ((h * 0.5) * Quat{0.0, d.ang.x, d.ang.y, d.ang.z}) * d.rot;
    d.rot = normalized_exact(d.rot + dq);

    f.cur = Frame{frame_origin(d.pos, d.rot, s.com), d.rot};
    return f;
}

// collision::ground + solver::solve for one body (src/collision.rs:13-35, src/solver.rs:19-27), in two passes.
//
// ground() only reads the post-integrate pose and the past frame, and solve() consumes the
// constraints in push order, so no constraint list is stored: constraint v is rebuilt from the
// frozen post-integrate frame `cur` and immediately projected onto the live pose (pos, rot).
// The arithmetic and its order per constraint are exactly the reference's.

// Pass 1 -- the `position.z >= 0.0` test of every vertex (src/collision.rs:17-18): bit v set <=> shape vertex v
// produces a constraint.  Only the z component of frame * vertex is live here, so the compiler drops the x/y
// arithmetic.  (A NaN height fails `>=` and therefore IS a contact, as in the reference.)
__device__ __forceinline__ uint32_t ground_mask(const Frame &cur, const double *verts, uint32_t n_verts)
{
    uint32_t mask = 0;
    for (uint32_t v = 0; v < n_verts; ++v) {
        const Vec3 vertex{verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
        const Vec3 x = cur * vertex;
        if (!(x.z >= 0.0))
            mask |= 1u << v;
    }
    return mask;
}

// Quat * Vec3 of xpbd_math.hpp for a v whose components are all below 2^970 in magnitude: the closing `c * 2.0 + v` in one
// fma per component.  Doubling is exact, so both forms round the same real number 2c + v -- unless 2c overflows
// (|c| >= 2^1023), where the plain form gives +-inf; then |2c + v| > 2^1024 - 2^970, the threshold from which rounding to
// nearest gives +-inf too.  NaN and inf in c behave alike in both forms.  So: the same bits for every c, with no guard, but
// only under the bound on v -- which the caller owes (k_step tests it once per kernel on a wave-uniform table; DESIGN
// section 2).  Every other rotation keeps the plain form.
__device__ __forceinline__ Vec3 rotate_bounded(Quat q, Vec3 v)
{
    const Vec3 qv = vec_of(q);
    const Vec3 t = cross(qv, v) + v * q.s;
    const Vec3 c = cross(qv, t);
    return Vec3{__builtin_fma(c.x, 2.0, v.x), __builtin_fma(c.y, 2.0, v.y), __builtin_fma(c.z, 2.0, v.z)};
}

// frame * vertex (src/frame.rs:47-53); BOUNDED: the vertex is an entry of a table that passed the 2^970 bound.
template <bool BOUNDED>
__device__ __forceinline__ Vec3 frame_times_vertex(const Frame &f, Vec3 vertex)
{
    return (BOUNDED ? rotate_bounded(f.rotation, vertex) : f.rotation * vertex) + f.position;
}

// Pass 1 for a wave whose lanes all have the same shape of exactly NV vertices: `table` holds that shape's vertices in
// wave-uniform values (k_step loads them once per kernel through a uniform address, so they live in scalar registers
// and feed the f64 instructions as scalar operands).  Fully unrolled: no LDS read and no per-lane loop in the substep.
// The expression per vertex is ground_mask's.  (k_step's grid path hands in a table rebuilt from a box's six distinct
// coordinates: the unrolled copies then repeat products on the same operands and the compiler keeps one of each.)
template <uint32_t NV, bool BOUNDED = false>
__device__ __forceinline__ uint32_t ground_mask_table(const Frame &cur, const double (&table)[3 * NV])
{
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t v = 0; v < NV; ++v) {
        const Vec3 vertex{table[3 * v + 0], table[3 * v + 1], table[3 * v + 2]};
        const Vec3 x = frame_times_vertex<BOUNDED>(cur, vertex);
        if (!(x.z >= 0.0))
            mask |= 1u << v;
    }
    return mask;
}

// The terrain's plane under world point x (include/xpbd.h, "TERRAIN", Lookup): false when x is outside the field (a NaN is).
// One division per axis, then one 32-byte load from the cell's 64-byte record: the planes themselves were evaluated once, by
// k_terrain_planes, with the header's formulas.  (Host code too: the terrain distance walk's CPU check runs it.)
XPBD_HD bool terrain_plane(const Terrain &t, const Vec3 &x, Plane &plane)
{
    const double u = (x.x - t.x0) / t.dx, v = (x.y - t.y0) / t.dy;
    if (!(u >= 0.0 && v >= 0.0))
        return false;
    const double fi = floor(u), fj = floor(v);
    if (!(fi < (double)(t.nx - 1) && fj < (double)(t.ny - 1))) // half-open at the far edges; only now are fi, fj known to fit
        return false;
    const uint32_t i = (uint32_t)fi, j = (uint32_t)fj;
    const double fu = u - fi, fv = v - fj;
    const double *p = t.planes + ((size_t)j * (t.nx - 1) + i) * 8 + (fu >= fv ? 0 : 4);
    plane = Plane{Vec3{p[0], p[1], p[2]}, p[3]};
    return true;
}

// Pass 1 on a terrain: vertex v contacts iff it is inside the field and below the plane under it.  (A vertex outside has no
// ground contact: beyond the terrain there is nothing.)
__device__ __forceinline__ uint32_t ground_mask_terrain(const Frame &cur, const double *verts, uint32_t n_verts, const Terrain &terrain)
{
    uint32_t mask = 0;
    for (uint32_t v = 0; v < n_verts; ++v) {
        const Vec3 vertex{verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
        const Vec3 x = cur * vertex;
        Plane plane;
        if (terrain_plane(terrain, x, plane) && !(distance(plane, x) >= 0.0))
            mask |= 1u << v;
    }
    return mask;
}

// The point of the terrain's plane below x: the `target` of a terrain contact.  (x is a vertex of the mask, so it is inside.)
__device__ __forceinline__ Vec3 terrain_target(const Terrain &terrain, const Vec3 &x)
{
    Plane plane{Vec3{0.0, 0.0, 1.0}, 0.0};
    (void)terrain_plane(terrain, x, plane);
    return x - distance(plane, x) * plane.normal;
}

// Pass 2 -- the lane walks the penetrating vertices of `mask` in ascending index order (the reference's push
// order).  Lane-compacting the contact work this way makes a wave run the expensive body max-over-lanes(contact
// count) times instead of once per shape vertex with most lanes masked off.  Recomputing x for the chosen vertex
// repeats the pass-1 arithmetic exactly, so the bits match.  (pos, rot) is the live pose the impulses act on.
// `limit` (> 0 only in XPBD_MODE_CONTACTS with xpbd_world_set_max_depenetration_speed; the pinned path passes the literal 0
// and compiles to the reference's arithmetic alone): the length of a ground constraint's correction is limited to
// max(0, limit - what the vertex has already moved towards its target in this substep), limit = speed * h.
// MATERIALS (XPBD_MODE_CONTACTS with xpbd_world_set_materials only; the pinned path compiles the plain form, where `mu` is
// never read and the reference's literal 1.0 stays a literal): Coulomb friction, mu = min(body, ground) -- the constraint
// takes back at most mu * |correction| of the tangential slip (include/xpbd.h, "Contact MATERIALS").
// TERRAIN (XPBD_MODE_CONTACTS with xpbd_world_set_terrain only; `mask` is then ground_mask_terrain's and every other form never
// reads `terrain`): the target is the point of the terrain's plane below the vertex instead of {x.x, x.y, 0.0}; the lookup
// repeats pass 1's on the same x, so the same plane.  Everything after `target` is the same arithmetic.
// BOUNDED_VERTS (k_step's grid path only): every entry of `verts` is below 2^970 in magnitude, so x takes rotate_bounded's
// single fma per component -- the same bits as the plain form.
template <bool MATERIALS = false, bool TERRAIN = false, bool BOUNDED_VERTS = false>
__device__ __forceinline__ void solve_masked(Vec3 &pos, Quat &rot, double inv_mass, const Mat3 &inv_inertia, const Vec3 &com,
                                             const Frame &cur, const Frame &past, double compliance, const double *verts,
                                             uint32_t mask, double limit = 0.0, double mu = 0.0, const Terrain &terrain = Terrain{})
{
    const Frame cur_inv = inverse(cur); // src/frame.rs:30-37, shared by every penetrating vertex
    for (uint32_t todo = mask; todo != 0; todo &= todo - 1) {
        const uint32_t v = __ffs(todo) - 1;
        const Vec3 vertex{verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
        const Vec3 x = frame_times_vertex<BOUNDED_VERTS>(cur, vertex); // src/collision.rs:17

        // src/collision.rs:22-29
        const Vec3 target = TERRAIN ? terrain_target(terrain, x) : Vec3{x.x, x.y, 0.0};
        const Vec3 correction = target - x;
        const Vec3 local = cur_inv * x;      // src/frame.rs:41
        const Vec3 delta = x - past * local; // src/frame.rs:42-43
        const Vec3 delta_tangential = delta - project_on(delta, correction);
        const Vec3 c0 = x;
        double k = 1.0;
        if (MATERIALS) {
            const double bound = mu * length(correction);
            const double len_t = length(delta_tangential);
            if (bound < len_t) // (false for mu = +inf, a NaN bound, len_t = 0: the reference's contact)
                k = bound / len_t;
        }
        const Vec3 c1 = target - k * delta_tangential;

        // solver::solve body, src/solver.rs:23-25 (distance == 0.0, src/collision.rs:30)
        const Vec3 difference = c1 - c0;                              // src/constraint.rs:13-15
        double current_distance, inv_distance; // length(difference), src/constraint.rs:21-23, and 1.0 / it
        exact::sqrt_and_reciprocal(length2(difference), current_distance, inv_distance);
        const Vec3 direction = difference * inv_distance; // src/constraint.rs:17-19
        // inverse_resitance, src/constraint.rs:25-32 (reads the LIVE pose)
        const Vec3 angular_impulse = conjugate(rot) * cross(c0 - (pos + com), direction);
        const double w = inv_mass + dot(inv_inertia * angular_impulse, angular_impulse);
        double error = current_distance;
        if (limit > 0.0) {
            const double len = length(correction);
            const double closing = len > 0.0 ? dot(delta, correction) / len : 0.0;
            double allowed = limit - closing;
            if (!(allowed > 0.0))
                allowed = 0.0;
            if (current_distance > allowed)
                error = allowed;
        }
        const double lagrange = (error - 0.0) / (w + compliance);
        // act -> apply_impulse, src/constraint.rs:34-37, src/rigid.rs:113-123
        const Vec3 impulse = lagrange * direction;
        pos = pos + impulse * inv_mass;
        const Vec3 arm = c0 - (pos + com);
        const Quat spin = quat_sv(0.0, cross(inv_inertia * arm, impulse));
        rot = rot + (0.5 * spin) * rot;
        rot = normalized_exact(rot);
    }
}

// Both passes for the lane's own body.  Returns the contact mask.
template <bool MATERIALS = false, bool TERRAIN = false>
__device__ __forceinline__ uint32_t solve_ground(BodyDynamic &d, const BodyStatic &s, const SubstepFrames &f,
                                                 double compliance, const double *verts, uint32_t n_verts, double limit = 0.0,
                                                 double mu = 0.0, const Terrain &terrain = Terrain{})
{
    const uint32_t mask = TERRAIN ? ground_mask_terrain(f.cur, verts, n_verts, terrain) : ground_mask(f.cur, verts, n_verts);
    solve_masked<MATERIALS, TERRAIN>(d.pos, d.rot, s.inv_mass, s.inv_inertia, s.com, f.cur, f.past, compliance, verts, mask, limit, mu,
                                     terrain);
    return mask;
}

// Rigid::derive, src/rigid.rs:101-109
__device__ __forceinline__ void derive_body(BodyDynamic &d, Vec3 past_pos, Quat past_rot, double h)
{
    d.vel = (d.pos - past_pos) / h;
    Quat dr = d.rot * conjugate(past_rot);
    if (dr.s < 0.0)
        dr = -dr;
    d.ang = (2.0 * vec_of(dr)) / h;
}

} // namespace xpbd
