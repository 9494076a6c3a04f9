// xpbd_contacts.hip -- body-body contact EXTENSION for gfx950: the per-substep contact pipeline
//     integrate + ground contacts  ->  wave-per-pair SAT  ->  Jacobi pair solve + derive.
// Semantics are defined by oracle/xpbd_pairs_oracle.h (op_contacts_step); the reference has no
// body-body contacts, so parity is UNPINNED.  The ground-contact part reuses the reference path
// (xpbd_step.hpp) unchanged.  The broadphase before it: xpbd_broadphase.hip; the velocity pass after it:
// xpbd_restitution.hip; what the units of the pipeline share: xpbd_contacts_device.hpp.
//
// Determinism: every floating-point sum is formed by ONE lane in a fixed order (neighbour index,
// then manifold point index); atomics are used on integers only (the statistics) and what they sum does not depend
// on the order.  Results do not depend on launch order or on how the world is sharded.
#include "xpbd_contacts_device.hpp"

namespace xpbd {
namespace {

// Worlds up to this many bodies run the pair solve with one lane per manifold POINT (eight lanes per body): below it
// the GPU is not full and a substep costs the dependent chain of one wave, which this shortens.
#ifndef XPBD_SMALL_WORLD
#define XPBD_SMALL_WORLD 16384
#endif
constexpr uint32_t kSmallWorld = XPBD_SMALL_WORLD;
#ifndef XPBD_PAIR_SOLVE_MIN_WAVES
#define XPBD_PAIR_SOLVE_MIN_WAVES 2
#endif

// Contact materials (include/xpbd.h, "Contact MATERIALS"): the coefficient of a contact is the smaller of its two sides'.
// (The coefficients are validated on the host: never NaN, so the comparison is an exact minimum.)
__device__ __forceinline__ double min_mu(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double ground_mu(const ContactBuffers &c, uint32_t i) { return min_mu(c.friction[i], c.ground_friction); }

// Body of work item `slot` under a BodySubset (false: nothing to do).
__device__ __forceinline__ bool subset_body(const BodySubset &ss, uint32_t n, uint32_t slot, uint32_t &i)
{
    if (ss.list) {
        if (slot >= ss.count)
            return false;
        i = ss.list[slot];
        return true;
    }
    i = slot;
    return slot < n && !(ss.skip && ss.skip[slot]);
}

// The 13 dynamic doubles of a body as one body-major row (halo buffers): position, rotation s x y z, velocity, angular velocity.
__device__ __forceinline__ void store_row(double *__restrict__ rows, uint32_t r, const BodyDynamic &d)
{
    double *o = rows + (size_t)r * kDynFields;
    o[0] = d.pos.x, o[1] = d.pos.y, o[2] = d.pos.z;
    o[3] = d.rot.s, o[4] = d.rot.x, o[5] = d.rot.y, o[6] = d.rot.z;
    o[7] = d.vel.x, o[8] = d.vel.y, o[9] = d.vel.z;
    o[10] = d.ang.x, o[11] = d.ang.y, o[12] = d.ang.z;
}

__device__ __forceinline__ BodyDynamic load_row(const double *__restrict__ rows, uint32_t r)
{
    const double *o = rows + (size_t)r * kDynFields;
    return BodyDynamic{Vec3{o[0], o[1], o[2]}, Quat{o[3], o[4], o[5], o[6]}, Vec3{o[7], o[8], o[9]}, Vec3{o[10], o[11], o[12]}};
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per body: integrate, remember the frames, ground contacts (reference path).
// ---------------------------------------------------------------------------------------------------
// MATERIALS: the form of a world with contact materials (c.friction set); the plain form never reads them.
// TERRAIN: the form of a world with a heightfield terrain (c.terrain.planes set): the ground contacts of xpbd_step.hpp's terrain forms.
template <bool TRACE, bool MATERIALS, bool TERRAIN = false>
__global__ void __launch_bounds__(kBlock) k_integrate_ground(BodyArrays b, ShapeTable shapes, double h, ContactBuffers c, BodySubset subset,
                                                             uint32_t *__restrict__ last_mask,
                                                             uint32_t *__restrict__ trace_masks, uint32_t trace_row)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_step
    uint32_t *lds_off = stage_shape_tables(lds, shapes);

    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t i;
    if (!subset_body(subset, b.n, slot, i))
        return;
    const uint32_t st = b.stride;
    const BodyStatic s = load_static(b, i);
    // (a ghost body starts the substep from its owner's end-of-substep state, straight from the gathered halo buffer)
    BodyDynamic d = subset.import_buf ? load_row(subset.import_buf, subset.import_rows[slot]) : load_dynamic(b.dyn, st, i);
    const uint32_t sid = b.shape_id[i];
    const uint32_t v0 = lds_off[sid];
    const double compliance = 1e-6 / (h * h);

    const SubstepFrames f = integrate_body(d, s, h);
    uint32_t mask;
    if (TERRAIN)
        mask = solve_ground<MATERIALS, true>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                             c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                             MATERIALS ? ground_mu(c, i) : 0.0, c.terrain);
    else
        mask = solve_ground<MATERIALS>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                       c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                       MATERIALS ? ground_mu(c, i) : 0.0);

    // the pose after the ground contacts lives in the record only: the pair solve (the one reader) takes it from there and
    // rewrites the whole SoA state (velocities come from derive)
    store_record(c.rec, i, f.cur, f.past, d.pos, d.rot, f.past_pos);
    last_mask[i] = mask;
    if (TRACE)
        trace_masks[(size_t)trace_row * st + i] = mask;
}

__global__ void k_body_frames(BodyArrays b, double *__restrict__ rec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b.n)
        store_record_p1(rec, i, body_frame(b, i));
}

__global__ void k_stat_records(BodyArrays b, double *__restrict__ stat_rec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t st = b.stride;
    double v[kStatRecDoubles] = {};
    v[0] = b.stat[(size_t)S_INV_MASS * st + i];
    for (uint32_t k = 0; k < 9; ++k)
        v[1 + k] = b.stat[(size_t)(S_INV_INERTIA + k) * st + i];
    for (uint32_t k = 0; k < 3; ++k)
        v[10 + k] = b.stat[(size_t)(S_COM + k) * st + i];
    double2 *r = reinterpret_cast<double2 *>(stat_rec + (size_t)i * kStatRecDoubles);
#pragma unroll
    for (uint32_t k = 0; k < kStatRecDoubles / 2; ++k)
        r[k] = double2{v[2 * k], v[2 * k + 1]};
}

// Rigid::frame() of every body, body-major (7 doubles each), staged through LDS so that the global
// stores are contiguous.
__global__ void __launch_bounds__(kBlock) k_body_frames_aos(BodyArrays b, double *__restrict__ frames)
{
    __shared__ double tile[kBlock * 7];
    const uint32_t base = blockIdx.x * kBlock, i = base + threadIdx.x;
    if (i < b.n) {
        const Frame f = body_frame(b, i);
        double *t = tile + threadIdx.x * 7;
        t[0] = f.position.x, t[1] = f.position.y, t[2] = f.position.z;
        t[3] = f.rotation.s, t[4] = f.rotation.x, t[5] = f.rotation.y, t[6] = f.rotation.z;
    }
    __syncthreads();
    const uint32_t count = min(kBlock, b.n - base);
    for (uint32_t k = threadIdx.x; k < count * 7; k += kBlock)
        frames[(size_t)base * 7 + k] = tile[k];
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per body: Jacobi over the pair contacts, then derive.
// ---------------------------------------------------------------------------------------------------
// What the pair solve needs of a body: pose after the ground contacts, mass properties, and its
// frames before / after this substep's integration.
struct PairBody {
    Vec3 pos;
    Quat rot;
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 com;
    Frame p1, past;
};

// The static fields of body i for its own integrate stage: mass properties from the StatRecord it has loaded anyway, the
// forces and torques (which nobody else reads) from the SoA arrays.
__device__ __forceinline__ BodyStatic static_of(const BodyArrays &b, uint32_t i, double inv_mass, const Mat3 &inv_inertia, Vec3 com)
{
    const uint32_t st = b.stride;
    BodyStatic s;
    s.inv_mass = inv_mass;
    s.inv_inertia = inv_inertia;
    s.com = com;
    s.ext_force = load3(b.stat, S_EXT_FORCE, st, i);
    s.int_force = load3(b.stat, S_INT_FORCE, st, i);
    s.ext_torque = load3(b.stat, S_EXT_TORQUE, st, i);
    s.int_torque = load3(b.stat, S_INT_TORQUE, st, i);
    return s;
}

// The BodyRecords of a workgroup's OWN bodies, staged in LDS (the per-body kernels with one lane per body and no body list):
// a body's neighbours are gathers of whole records -- 2 x 128-byte lines each -- and in an index-coherent scene (box stacks: a
// column is 16 consecutive bodies) most of them are bodies of the same workgroup, whose records the workgroup has loaded once
// already.  PMC on `stacks` (profiles/r02_c): 373 MB read per launch for ~160 MB of distinct data, the kernel at the gather
// rate of the memory system (5.3 TB/s of lines).  Word k of the record of the workgroup's body t sits at words[k * kBlock + t]:
// consecutive lanes read consecutive 16-byte words (no bank conflicts).  Same values from another place: same bits.
#ifndef XPBD_PAIR_SOLVE_STAGE_RECORDS
#define XPBD_PAIR_SOLVE_STAGE_RECORDS 0 // measured and rejected, see DESIGN.md 8 (the fetched bytes of the kernel fall by 29 % on box stacks, its time does not)
#endif
struct RecordStage {
    const double2 *words = nullptr; // LDS; null = not staged
    uint32_t first = 0, count = 0;  // bodies [first, first + count) are staged
};

__device__ __forceinline__ BodyRecord load_record_staged(const double *__restrict__ rec, uint32_t i, const RecordStage &stage)
{
    const uint32_t t = i - stage.first;
    if (stage.words && t < stage.count) {
        double2 v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            v[k] = stage.words[k * kBlock + t];
        BodyRecord o;
        o.p1 = Frame{Vec3{v[0].x, v[0].y, v[1].x}, Quat{v[1].y, v[2].x, v[2].y, v[3].x}};
        o.past = Frame{Vec3{v[3].y, v[4].x, v[4].y}, Quat{v[5].x, v[5].y, v[6].x, v[6].y}};
        o.pos = Vec3{v[7].x, v[7].y, v[8].x};
        o.rot = Quat{v[8].y, v[9].x, v[9].y, v[10].x};
        o.past_pos = Vec3{v[10].y, v[11].x, v[11].y};
        return o;
    }
    return load_record(rec, i);
}

// Every thread of the workgroup calls this (it ends in a barrier): thread t stages the record of body `first + t`.
__device__ __forceinline__ RecordStage stage_records(double2 *__restrict__ words, const double *__restrict__ rec, uint32_t first, uint32_t n)
{
    const uint32_t t = threadIdx.x, i = first + t;
    if (i < n) {
        const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kRecDoubles);
        double2 v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            v[k] = r[k];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            words[k * kBlock + t] = v[k];
    }
    __syncthreads();
    RecordStage s;
    s.words = words;
    s.first = first;
    s.count = n > first ? (n - first < kBlock ? n - first : kBlock) : 0u;
    return s;
}

// (past_pos: optional, the position before integrate -- only a body's own derive needs it)
__device__ __forceinline__ PairBody load_pair_body(const ContactBuffers &c, uint32_t i, Vec3 *past_pos = nullptr,
                                                   const RecordStage &stage = RecordStage())
{
    const BodyRecord r = load_record_staged(c.rec, i, stage); // two cache lines, or LDS
    const StatRecord s = load_stat_record(c.stat_rec, c.stat_index ? c.stat_index[i] : i); // one, or a cached table entry
    PairBody p;
    p.pos = r.pos;
    p.rot = r.rot;
    p.inv_mass = s.inv_mass;
    p.inv_inertia = s.inv_inertia;
    p.com = s.com;
    p.p1 = r.p1;
    p.past = r.past;
    if (past_pos)
        *past_pos = r.past_pos;
    return p;
}

// Frame::delta, src/frame.rs:40-44
__device__ __forceinline__ Vec3 frame_delta(const Frame &cur, const Frame &past, Vec3 global)
{
    const Vec3 local = inverse(cur) * global;
    return global - past * local;
}

// The angular limits of joint `joint` for body `self` (xpbd.h, XPBD_LIMIT_*): every limit that binds is a Jacobi entry of its
// own, in the caller's order.  Evaluated per body like the hinge's angular term, 3-vectors selected by role (a / b), so both
// ends of the joint compute the same phi, n and lambda.  A limit that does not bind adds nothing, not even to `count`.
#ifndef XPBD_JOINT_LIMIT_INLINE
#define XPBD_JOINT_LIMIT_INLINE __forceinline__
#endif
__device__ XPBD_JOINT_LIMIT_INLINE void joint_limit_terms(const ContactBuffers &c, uint32_t joint, const Joint &jt, bool self_is_a,
                                                          const PairBody &self, const PairBody &other, double compliance, Quat &drot,
                                                          uint32_t &count)
{
    const uint32_t l_end = c.limit_off[joint + 1];
    for (uint32_t l = c.limit_off[joint]; l < l_end; ++l) {
        const JointLimit &lim = c.limits[l];
        const Quat q_a = self_is_a ? self.rot : other.rot, q_b = self_is_a ? other.rot : self.rot;
        const Vec3 a_w = q_a * Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
        double phi;
        Vec3 n;
        if (lim.kind == XPBD_LIMIT_SWING) {
            const Vec3 b_w = q_b * Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
            const Vec3 cr = cross(a_w, b_w);
            const double s = length(cr);
            if (s == 0.0)
                continue;
            phi = atan2(s, dot(a_w, b_w));
            n = cr * (1.0 / s);
        } else {
            Vec3 p_a = q_a * Vec3{lim.ref_a[0], lim.ref_a[1], lim.ref_a[2]};
            Vec3 p_b = q_b * Vec3{lim.ref_b[0], lim.ref_b[1], lim.ref_b[2]};
            if (lim.kind == XPBD_LIMIT_HINGE) {
                n = a_w;
            } else { // XPBD_LIMIT_TWIST: about the bisector of the two axes, on the references' projections
                const Vec3 bisector = a_w + q_b * Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
                const double len = length(bisector);
                if (len == 0.0)
                    continue;
                n = bisector * (1.0 / len);
                p_a = p_a - n * dot(p_a, n);
                p_b = p_b - n * dot(p_b, n);
            }
            phi = atan2(dot(cross(p_a, p_b), n), dot(p_a, p_b));
        }
        const double clamped = phi < lim.lower ? lim.lower : (phi > lim.upper ? lim.upper : phi);
        const double err = phi - clamped;
        if (err == 0.0)
            continue;
        const Vec3 n_self = conjugate(self.rot) * n, n_other = conjugate(other.rot) * n;
        const double w_s = dot(self.inv_inertia * n_self, n_self), w_o = dot(other.inv_inertia * n_other, n_other);
        const double w = self_is_a ? w_s + w_o : w_o + w_s; // w_a + w_b
        const double lambda = err / (w + compliance);
        const Vec3 turn = self_is_a ? lambda * n : (-lambda) * n;
        const Quat spin = quat_sv(0.0, self.inv_inertia * turn);
        drot = drot + (0.5 * spin) * self.rot;
        ++count;
    }
}

// Jacobi pair solve + joints + derive of body i: its state at the end of the substep.
// (touching, points: += the manifolds with contact points among this body's pairs (i, j > i) and their points -- every
// pair is counted by its smaller body, which gives the pipeline's statistics without a pass of their own)
//
// G = lanes per body.  G = 1: the lane walks the points of a manifold one after the other.  G = 8 (small worlds, where
// a wave's dependent chain is the whole cost): lane `sub` evaluates point `sub` of the manifold, and the terms are then
// added on every lane in point order -- the same values in the same order, so the same bits.
#ifndef XPBD_PAIR_SOLVE_ROUND_POINTS
#define XPBD_PAIR_SOLVE_ROUND_POINTS 2 // points of a manifold per round, see pass 2 below; A/B (boxes pile / mixed pile SAT / GJK+EPA,
                                       // 1e8 body-substeps/s): 1 point 5.24 / 2.56 / 2.76, 2 points 5.35 / 2.57 / 2.80, 3 points 5.30 / 2.54 / 2.75
#endif
// MATERIALS: contact materials are set (c.friction; uniform over the launch, chosen by the launcher).  The plain form is the
// reference's contact: it loads no coefficient and keeps the literal 1.0.
template <uint32_t G, bool MATERIALS>
__device__ __forceinline__ BodyDynamic pair_solve_derive_body(const ContactBuffers &c, uint32_t i, double h,
                                                              const PairBody &self, Vec3 self_past_pos, uint32_t sub, uint32_t &touching,
                                                              uint32_t &points, const RecordStage &stage = RecordStage())
{
    static_assert(G == 1 || G == kMaxManifoldPoints, "one lane per body or one lane per manifold point");
    const double compliance = 1e-6 / (h * h);
    const double limit = c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0;
    const double mu_self = MATERIALS ? c.friction[i] : 0.0;

    Vec3 dpos{0.0, 0.0, 0.0};
    Quat drot{0.0, 0.0, 0.0, 0.0};
    uint32_t count = 0;
    // One neighbour with contact points: its points' terms added in point order.
    auto neighbour_terms = [&](uint32_t j, const ContactManifold *m, uint32_t n_points, uint32_t feature, uint32_t pt_begin, uint32_t pt_end) {
        if (j > i && pt_begin == 0) {
            ++touching;
            points += n_points;
        }
        const PairBody other = load_pair_body(c, j, nullptr, stage);
        const double mu = MATERIALS ? min_mu(mu_self, c.friction[j]) : 0.0; // (only touching neighbours get here)
        // pair (A, B) = (min, max); the reference body is A unless the reference face is on B.  The formulas are
        // written in terms of the incident and the reference body; here every term is evaluated for `self` and
        // `other` with their own point and only 3-vectors are selected by role -- selecting whole bodies by a
        // per-lane condition made the compiler keep four body records live (255 VGPRs + AGPRs, one wave per SIMD).
        const bool self_is_a = i < j;
        const bool ref_is_a = feature != 1u;
        const bool self_is_inc = self_is_a != ref_is_a;
        // a face contact stores its reference plane and the points on the incident body; their partners on the reference
        // body are the clipper's projections, re-evaluated with its own expression (xpbd_clip.hpp: Plane::project) -- the
        // same inputs through the same operations, so the same bits.  Feature 2: the single contact's two points.
        const bool face = feature != 2u;
        const Plane ref_plane{Vec3{m->plane[0], m->plane[1], m->plane[2]}, m->plane[3]};
        // one contact point: what it adds to dpos and drot
        auto point_term = [&](uint32_t pt, Vec3 &term_pos, Quat &term_rot) {
            const Vec3 p_inc{m->point[pt][0], m->point[pt][1], m->point[pt][2]};
            Vec3 p_ref;
            if (face) {
                const double depth = distance(ref_plane, p_inc);
                p_ref = p_inc - depth * ref_plane.normal;
            } else {
                p_ref = Vec3{m->point[1][0], m->point[1][1], m->point[1][2]};
            }
            const Vec3 p_self = self_is_inc ? p_inc : p_ref, p_other = self_is_inc ? p_ref : p_inc;
            const Vec3 correction = p_ref - p_inc;
            const Vec3 moved_self = frame_delta(self.p1, self.past, p_self), moved_other = frame_delta(other.p1, other.past, p_other);
            const Vec3 delta_rel = self_is_inc ? moved_self - moved_other : moved_other - moved_self; // incident - reference
            const Vec3 delta_tangential = delta_rel - project_on(delta_rel, correction);
            const Vec3 c0 = p_inc;
            double k = 1.0;
            if (MATERIALS) { // Coulomb's cone on positions: at most mu * |correction| of the tangential slip is taken back
                const double bound = mu * length(correction);
                const double len_t = length(delta_tangential);
                if (bound < len_t) // (false for mu = +inf, a NaN bound, len_t = 0: the reference's contact)
                    k = bound / len_t;
            }
            const Vec3 c1 = p_ref - k * delta_tangential;
            const Vec3 difference = c1 - c0;
            const double dist = length(difference);
            const Vec3 dir = difference * (1.0 / dist);
            // w = w_incident + w_reference; IEEE addition commutes, so the order of the two bodies does not matter
            const double w = generalized_inverse_mass(self, p_self, dir) + generalized_inverse_mass(other, p_other, dir);
            double error = dist;
            if (limit > 0.0) { // xpbd_world_set_max_depenetration_speed (uniform over the launch; 0 = off); oracle: accumulate_point
                const double len = length(correction);
                const double closing = len > 0.0 ? dot(delta_rel, correction) / len : 0.0;
                double allowed = limit - closing;
                if (!(allowed > 0.0))
                    allowed = 0.0;
                if (dist > allowed)
                    error = allowed;
            }
            const double lambda = (error - 0.0) / (w + compliance);

            const Vec3 impulse = self_is_inc ? lambda * dir : (-lambda) * dir;
            term_pos = impulse * self.inv_mass;
            const Vec3 arm = p_self - (self.pos + self.com);
            const Quat spin = quat_sv(0.0, cross(self.inv_inertia * arm, impulse));
            term_rot = (0.5 * spin) * self.rot;
        };
        if (G == 1) {
            for (uint32_t pt = pt_begin; pt < pt_end; ++pt) {
                Vec3 term_pos;
                Quat term_rot;
                point_term(pt, term_pos, term_rot);
                dpos = dpos + term_pos;
                drot = drot + term_rot;
                ++count;
            }
        } else {
            Vec3 term_pos{0.0, 0.0, 0.0};
            Quat term_rot{0.0, 0.0, 0.0, 0.0};
            if (sub < n_points)
                point_term(sub, term_pos, term_rot);
            for (uint32_t pt = 0; pt < n_points; ++pt) { // every lane of the group adds the terms in point order
                dpos = dpos + Vec3{__shfl(term_pos.x, pt, G), __shfl(term_pos.y, pt, G), __shfl(term_pos.z, pt, G)};
                drot = drot + Quat{__shfl(term_rot.s, pt, G), __shfl(term_rot.x, pt, G), __shfl(term_rot.y, pt, G),
                                   __shfl(term_rot.z, pt, G)};
                ++count;
            }
        }
    };
    // Pass 1 -- which of the body's neighbour slots have contact points: bit u of `touch` = slot k_begin + u.  The
    // neighbours in batches of four: their pair indices, then their point counts, are fetched side by side, so a body
    // pays two dependent round trips per batch instead of two per neighbour (most neighbours of a loose scene do not
    // touch, and the whole cost of looking at them is that latency).
    // Pass 2 -- the lanes of a wave then walk THEIR OWN touching neighbours, round by round (ascending, so every body
    // still adds its terms in the oracle's order): a wave runs as many rounds as its busiest body has touching
    // neighbours.  Walking the slots in lockstep instead made it run every slot that any of its 64 bodies had a
    // contact in -- in a settled pile of boxes (7.8 neighbours a body, 3.2 of them touching) 14 slots with four lanes in
    // ten idle in each: 17 % lane utilisation (PMC), 19 000 VALU instructions per wave.
    const uint32_t k_end = c.nbr_off[i + 1];
    for (uint32_t k_base = c.nbr_off[i]; k_base < k_end; k_base += 64) { // (64 slots per mask: one trip for all but monsters)
        const uint32_t k_stop = k_end - k_base > 64u ? k_base + 64u : k_end;
        unsigned long long touch = 0;
        // (a wave whose bodies all have one or two neighbours -- box stacks -- skips pass 1: nothing to filter there)
        const bool few = __all(k_stop - k_base <= 2u);
        if (few)
            touch = k_stop - k_base == 2u ? 3ull : 1ull;
        for (uint32_t k0 = k_base; !few && k0 < k_stop; k0 += 4) {
            uint32_t pair_of[4], points_of[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                pair_of[u] = k0 + u < k_stop ? c.nbr_pair[k0 + u] : 0u;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                points_of[u] = k0 + u < k_stop ? (uint32_t)c.pair_codes[pair_of[u]] : 0u;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                if (points_of[u])
                    touch |= 1ull << (k0 - k_base + u);
        }
        // (the next neighbour and its pair index are fetched while the current one's points are evaluated)
        uint32_t j_next = 0, pair_next = 0;
        if (touch) {
            const uint32_t k = k_base + (uint32_t)__ffsll((long long)touch) - 1u;
            j_next = c.nbr[k], pair_next = c.nbr_pair[k];
        }
        // A round takes at most `chunk` points of a manifold; a longer manifold goes on in the lane's next round.  The
        // rounds of a wave are as long as their longest share, and in a pile the manifolds have 1.4 points on average but
        // four in the longest: with whole manifolds per round the lanes idled through two thirds of every round (PMC:
        // 26 % lane utilisation).  Stacks (every manifold four points) take them whole.  G lanes per body: one point per lane.
        const uint32_t chunk = (G > 1 || few) ? kMaxManifoldPoints : (uint32_t)XPBD_PAIR_SOLVE_ROUND_POINTS;
        uint32_t j_cur = 0, pair_cur = 0, code_cur = 0, n_cur = 0, pt = 0;
        while (touch || pt < n_cur) {
            if (pt == n_cur) { // this lane's next touching neighbour
                j_cur = j_next, pair_cur = pair_next;
                touch &= touch - 1ull;
                if (touch) {
                    const uint32_t k = k_base + (uint32_t)__ffsll((long long)touch) - 1u;
                    j_next = c.nbr[k], pair_next = c.nbr_pair[k];
                }
                code_cur = c.pair_codes[pair_cur];
                n_cur = code_cur & ((1u << kPairCodeFeatureShift) - 1u);
                pt = 0;
            }
            if (n_cur) { // (zero only after the shortcut above: a listed neighbour that does not touch)
                const uint32_t stop = n_cur - pt > chunk ? pt + chunk : n_cur;
                neighbour_terms(j_cur, c.manifolds + pair_cur, n_cur, code_cur >> kPairCodeFeatureShift, pt, stop);
                pt = stop;
            }
        }
    }

    // joints of this body, ascending joint index (same accumulator: the "mixed-constraint" pass)
    if (c.joint_off) {
        for (uint32_t k = c.joint_off[i]; k < c.joint_off[i + 1]; ++k) {
            const Joint &jt = c.joints[c.joint_list[k]];
            const bool self_is_a = jt.body_a == i;
            const PairBody other = load_pair_body(c, self_is_a ? jt.body_b : jt.body_a, nullptr, stage);
            // as above: evaluate per body, select 3-vectors by role (a / b)
            const Vec3 anchor_self = self_is_a ? Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]} : Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]};
            const Vec3 anchor_other = self_is_a ? Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]} : Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]};
            const Vec3 p_self = Frame{frame_origin(self.pos, self.rot, self.com), self.rot} * anchor_self;
            const Vec3 p_other = Frame{frame_origin(other.pos, other.rot, other.com), other.rot} * anchor_other;
            const Vec3 difference = self_is_a ? p_other - p_self : p_self - p_other; // p_b - p_a
            const double dist = length(difference);
            // (coincident points: the reference's direction() would be NaN (K6); nothing to correct.  A slider has no
            // positional term: its anchor is held to the axis by k_joint_extras)
            if (dist != 0.0 && jt.kind != XPBD_JOINT_SLIDER) {
                const Vec3 dir = difference * (1.0 / dist);
                const double w = generalized_inverse_mass(self, p_self, dir) + generalized_inverse_mass(other, p_other, dir);
                const double lambda = (dist - jt.distance) / (w + compliance);
                const Vec3 impulse = self_is_a ? lambda * dir : (-lambda) * dir;
                dpos = dpos + impulse * self.inv_mass;
                const Vec3 arm = p_self - (self.pos + self.com);
                const Quat spin = quat_sv(0.0, cross(self.inv_inertia * arm, impulse));
                drot = drot + (0.5 * spin) * self.rot;
                ++count;
            }
            if (jt.kind != XPBD_JOINT_DISTANCE) { // XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER
                // the angular term (oracle: accumulate_hinge): the joint's axes, unit vectors in the object space of a and b,
                // are kept aligned; evaluated per body, 3-vectors selected by role as above
                const Vec3 axis_self = self_is_a ? Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]} : Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
                const Vec3 axis_other = self_is_a ? Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]} : Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
                const Vec3 w_self = self.rot * axis_self, w_other = other.rot * axis_other;
                const Vec3 delta = self_is_a ? cross(w_self, w_other) : cross(w_other, w_self); // a_w x b_w
                const double mag = length(delta);
                if (mag != 0.0) {
                    const Vec3 n = delta * (1.0 / mag);
                    const Vec3 n_self = conjugate(self.rot) * n, n_other = conjugate(other.rot) * n;
                    const double w_s = dot(self.inv_inertia * n_self, n_self), w_o = dot(other.inv_inertia * n_other, n_other);
                    const double w = self_is_a ? w_s + w_o : w_o + w_s; // w_a + w_b (IEEE addition commutes; written out for the reader)
                    const double lambda = mag / (w + compliance);
                    const Vec3 turn = self_is_a ? lambda * n : (-lambda) * n;
                    const Quat spin = quat_sv(0.0, self.inv_inertia * turn);
                    drot = drot + (0.5 * spin) * self.rot;
                    ++count;
                }
            }
            if (c.limit_off)
                joint_limit_terms(c, c.joint_list[k], jt, self_is_a, self, other, compliance, drot, count);
            if (c.joint_extra) { // the joint's extra entries for this end, summed by k_joint_extras into the record of this
                                 // slot of the body's joint list (zero count: none; adding zeros could flip the sign of a zero)
                const double *e = c.joint_extra + (size_t)k * kJointExtraDoubles;
                if (e[7] != 0.0) {
                    dpos = dpos + Vec3{e[0], e[1], e[2]};
                    drot = drot + Quat{e[3], e[4], e[5], e[6]};
                    count += (uint32_t)e[7];
                }
            }
        }
    }

    BodyDynamic d;
    d.pos = self.pos;
    d.rot = self.rot;
    if (count) {
        const double cnt = (double)count;
        d.pos = self.pos + dpos / cnt;
        d.rot = normalized(self.rot + Quat{drot.s / cnt, drot.x / cnt, drot.y / cnt, drot.z / cnt});
    }
    derive_body(d, self_past_pos, self.past.rotation, h);
    return d;
}

// stats[0] += touching, stats[1] += points, summed over the workgroup: TWO atomics per workgroup (same-address atomics
// serialise at ~10-25 ns each -- never one per pair, see xpbd_pairs.hip).  Every thread of the block must call this.
__device__ __forceinline__ void block_add_stats(uint32_t touching, uint32_t points, unsigned long long *__restrict__ stats)
{
    for (uint32_t off = 32; off; off >>= 1) {
        touching += __shfl_xor(touching, off, 64);
        points += __shfl_xor(points, off, 64);
    }
    __shared__ uint32_t part[2][kBlock / 64];
    if ((threadIdx.x & 63u) == 0) {
        part[0][threadIdx.x >> 6] = touching;
        part[1][threadIdx.x >> 6] = points;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0, p = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            t += part[0][w];
            p += part[1][w];
        }
        if (t)
            atomicAdd(&stats[0], (unsigned long long)t);
        if (p)
            atomicAdd(&stats[1], (unsigned long long)p);
    }
}

template <uint32_t G, bool MATERIALS>
__global__ void __launch_bounds__(kBlock, XPBD_PAIR_SOLVE_MIN_WAVES) k_pair_solve_derive(BodyArrays b, double *__restrict__ dyn_out, double h,
                                                                                        ContactBuffers c, BodySubset subset)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, slot = gid / G, sub = gid % G;
    // one lane per body, bodies in index order: the workgroup's own records go through LDS (load_record_staged)
    constexpr bool kStage = G == 1 && XPBD_PAIR_SOLVE_STAGE_RECORDS;
    __shared__ double2 stage_words[kStage ? 12 * kBlock : 1];
    RecordStage stage;
    if (kStage && !subset.list)
        stage = stage_records(stage_words, c.rec, blockIdx.x * kBlock, b.n);
    uint32_t touching = 0, points = 0, i;
    if (subset_body(subset, b.n, slot, i)) {
        Vec3 past_pos;
        const PairBody self = load_pair_body(c, i, &past_pos, stage);
        const BodyDynamic d = pair_solve_derive_body<G, MATERIALS>(c, i, h, self, past_pos, sub, touching, points, stage);
        if (sub == 0) {
            store_dynamic(dyn_out, b.stride, i, d);
            if (subset.export_rows)
                store_row(subset.export_rows, slot, d);
        }
    }
    block_add_stats(sub == 0 ? touching : 0u, sub == 0 ? points : 0u, c.stats);
}

// The end of substep k and the beginning of substep k + 1 of one body in one kernel: pair solve + derive, then
// integrate + ground contacts straight from registers.  Nothing a body needs from the others changes in between
// (they read each other's state of substep k: dyn and the frames of `c`), so the new state goes to the other dyn
// buffer and the frames of substep k + 1 to the other frame set (`next`).  Saves the store + reload of the dynamic
// state, half of the static loads and one launch per substep; same arithmetic, same bits.  Only for step calls
// that run all their substeps on one device: a halo exchange sits exactly at this seam.
// (G lanes per body as in pair_solve_derive_body; with G = 8 the integrate + ground part runs redundantly on the eight
// lanes and lane 0 stores.)
template <bool TRACE, uint32_t G, bool MATERIALS>
__global__ void __launch_bounds__(kBlock, XPBD_PAIR_SOLVE_MIN_WAVES) k_pair_solve_integrate_ground(
    BodyArrays b, ShapeTable shapes, double h, ContactBuffers c, BodySubset subset, double *__restrict__ next_rec,
    uint32_t *__restrict__ last_mask, uint32_t *__restrict__ trace_masks, uint32_t trace_row)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_integrate_ground
    uint32_t *lds_off = stage_shape_tables(lds, shapes);

    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, slot = gid / G, sub = gid % G;
    constexpr bool kStage = G == 1 && XPBD_PAIR_SOLVE_STAGE_RECORDS; // see k_pair_solve_derive
    __shared__ double2 stage_words[kStage ? 12 * kBlock : 1];
    RecordStage stage;
    if (kStage && !subset.list)
        stage = stage_records(stage_words, c.rec, blockIdx.x * kBlock, b.n);
    uint32_t touching = 0, points = 0, i;
    if (subset_body(subset, b.n, slot, i)) {
        const uint32_t st = b.stride;
        BodyDynamic d;
        BodyStatic s;
        {
            Vec3 past_pos;
            const PairBody self = load_pair_body(c, i, &past_pos, stage);
            d = pair_solve_derive_body<G, MATERIALS>(c, i, h, self, past_pos, sub, touching, points, stage);
            s = static_of(b, i, self.inv_mass, self.inv_inertia, self.com);
        }
        if (subset.export_rows && sub == 0)
            store_row(subset.export_rows, slot, d); // the end-of-substep state, before the next substep's integration
        const uint32_t sid = b.shape_id[i];
        const uint32_t v0 = lds_off[sid];
        const double compliance = 1e-6 / (h * h);
        const SubstepFrames f = integrate_body(d, s, h);
        const uint32_t mask = solve_ground<MATERIALS>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                                      c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                                      MATERIALS ? ground_mu(c, i) : 0.0);
        if (sub == 0) {
            // everything the next kernel needs of this body is its record: no SoA state is written between the substeps of
            // a step call (the last substep's k_pair_solve_derive writes all 13 dynamic fields)
            store_record(next_rec, i, f.cur, f.past, d.pos, d.rot, f.past_pos);
            last_mask[i] = mask;
            if (TRACE)
                trace_masks[(size_t)trace_row * st + i] = mask;
        }
    }
    block_add_stats(sub == 0 ? touching : 0u, sub == 0 ? points : 0u, c.stats);
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per joint with extras: sliders and joint drives (include/xpbd.h, "SLIDERS and joint DRIVES").
// ---------------------------------------------------------------------------------------------------
// The summed extra entries of one joint end.
struct ExtraSum {
    Vec3 dpos{0.0, 0.0, 0.0};
    Quat drot{0.0, 0.0, 0.0, 0.0};
    uint32_t count = 0;
};

// One linear entry: the impulse +lambda n on a at p_a, -lambda n on b at p_b, applied as the positional term applies its own.
__device__ __forceinline__ void extra_linear_entry(const PairBody &a, const PairBody &b, Vec3 p_a, Vec3 p_b, Vec3 n, double lambda, ExtraSum &sum_a,
                                                   ExtraSum &sum_b)
{
    const Vec3 impulse_a = lambda * n, impulse_b = (-lambda) * n;
    sum_a.dpos = sum_a.dpos + impulse_a * a.inv_mass;
    sum_b.dpos = sum_b.dpos + impulse_b * b.inv_mass;
    const Vec3 arm_a = p_a - (a.pos + a.com), arm_b = p_b - (b.pos + b.com);
    const Quat spin_a = quat_sv(0.0, cross(a.inv_inertia * arm_a, impulse_a)), spin_b = quat_sv(0.0, cross(b.inv_inertia * arm_b, impulse_b));
    sum_a.drot = sum_a.drot + (0.5 * spin_a) * a.rot;
    sum_b.drot = sum_b.drot + (0.5 * spin_b) * b.rot;
    ++sum_a.count;
    ++sum_b.count;
}

// One angular entry: a turns by +lambda n, b by -lambda n, as a limit's entry does.
__device__ __forceinline__ void extra_angular_entry(const PairBody &a, const PairBody &b, Vec3 n, double lambda, ExtraSum &sum_a, ExtraSum &sum_b)
{
    const Quat spin_a = quat_sv(0.0, a.inv_inertia * (lambda * n)), spin_b = quat_sv(0.0, b.inv_inertia * ((-lambda) * n));
    sum_a.drot = sum_a.drot + (0.5 * spin_a) * a.rot;
    sum_b.drot = sum_b.drot + (0.5 * spin_b) * b.rot;
    ++sum_a.count;
    ++sum_b.count;
}

__device__ __forceinline__ double wrap_angle(double x)
{
    const double pi = 3.14159265358979323846;
    return x > pi ? x - 2.0 * pi : (x < -pi ? x + 2.0 * pi : x);
}

__device__ __forceinline__ void store_extra_sum(double *__restrict__ out, const ExtraSum &s)
{
    double2 *o = reinterpret_cast<double2 *>(out);
    o[0] = double2{s.dpos.x, s.dpos.y};
    o[1] = double2{s.dpos.z, s.drot.s};
    o[2] = double2{s.drot.x, s.drot.y};
    o[3] = double2{s.drot.z, (double)s.count};
}

// One lane per joint with extras.  Both ends are loaded from the records of this substep and every term is evaluated ONCE,
// so both ends get the same phi, n and lambda; the two sums go to the records of the joint's two slots in the bodies' joint
// lists (c.extra_slots), where the pair solve of the same substep picks them up.  Nothing here is read by another lane of the launch.
__global__ void __launch_bounds__(kBlock) k_joint_extras(double h, ContactBuffers c)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= c.n_extra_joints)
        return;
    const uint32_t joint = c.extra_joints[t];
    const Joint &jt = c.joints[joint];
    const PairBody a = load_pair_body(c, jt.body_a), b = load_pair_body(c, jt.body_b);
    const double hh = h * h;
    const double compliance = 1e-6 / hh;
    const Vec3 anchor_a{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]}, anchor_b{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]};
    const Vec3 axis_a{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
    const Vec3 p_a = Frame{frame_origin(a.pos, a.rot, a.com), a.rot} * anchor_a;
    const Vec3 p_b = Frame{frame_origin(b.pos, b.rot, b.com), b.rot} * anchor_b;
    const Vec3 d = p_b - p_a;
    const Vec3 a_w = a.rot * axis_a;
    const double s = dot(d, a_w);
    ExtraSum sum_a, sum_b;

    if (jt.kind == XPBD_JOINT_SLIDER) { // 1. the anchor of b is held to the axis of a
        const Vec3 r = d - a_w * s;
        const double len = length(r);
        if (len != 0.0) {
            const Vec3 n = r * (1.0 / len);
            const double w = generalized_inverse_mass(a, p_a, n) + generalized_inverse_mass(b, p_b, n);
            extra_linear_entry(a, b, p_a, p_b, n, len / (w + compliance), sum_a, sum_b);
        }
    }
    const uint32_t k_end = c.extra_off[t + 1];
    for (uint32_t k = c.extra_off[t]; k < k_end; ++k) { // 2. the SLIDE limit, 3. the drives in the caller's order
        const JointExtraItem &it = c.extra_items[k];
        const bool angular = it.kind == XPBD_DRIVE_ANGLE || it.kind == XPBD_DRIVE_ANGULAR_VELOCITY;
        double err, w;
        if (angular) {
            const Vec3 ref_a{it.ref_a[0], it.ref_a[1], it.ref_a[2]}, ref_b{it.ref_b[0], it.ref_b[1], it.ref_b[2]};
            const Vec3 r_a = a.rot * ref_a, r_b = b.rot * ref_b;
            const double phi = atan2(dot(cross(r_a, r_b), a_w), dot(r_a, r_b)); // as XPBD_LIMIT_HINGE
            if (it.kind == XPBD_DRIVE_ANGLE) {
                err = wrap_angle(phi - it.target);
            } else { // the same angle at the start of the substep
                const Vec3 a_w0 = a.past.rotation * axis_a;
                const Vec3 r_a0 = a.past.rotation * ref_a, r_b0 = b.past.rotation * ref_b;
                const double phi0 = atan2(dot(cross(r_a0, r_b0), a_w0), dot(r_a0, r_b0));
                err = wrap_angle(phi - phi0) - it.target * h;
            }
            const Vec3 n_a = conjugate(a.rot) * a_w, n_b = conjugate(b.rot) * a_w;
            w = dot(a.inv_inertia * n_a, n_a) + dot(b.inv_inertia * n_b, n_b);
        } else {
            if (it.kind == kExtraSlideLimit) {
                const double clamped = s < it.target ? it.target : (s > it.compliance ? it.compliance : s); // lower, upper
                err = s - clamped;
            } else if (it.kind == XPBD_DRIVE_POSITION) {
                err = s - it.target;
            } else { // XPBD_DRIVE_VELOCITY: the same offset at the start of the substep
                const Vec3 d0 = b.past * anchor_b - a.past * anchor_a;
                const double s0 = dot(d0, a.past.rotation * axis_a);
                err = (s - s0) - it.target * h;
            }
            w = generalized_inverse_mass(a, p_a, a_w) + generalized_inverse_mass(b, p_b, a_w);
        }
        if (err == 0.0)
            continue;
        double lambda;
        if (it.kind == kExtraSlideLimit) {
            lambda = err / (w + compliance);
        } else {
            lambda = err / (w + (1e-6 + it.compliance) / hh);
            const double cap = it.max_force * hh;
            lambda = lambda > cap ? cap : (lambda < -cap ? -cap : lambda);
        }
        if (angular)
            extra_angular_entry(a, b, a_w, lambda, sum_a, sum_b);
        else
            extra_linear_entry(a, b, p_a, p_b, a_w, lambda, sum_a, sum_b);
    }
    store_extra_sum(c.joint_extra + (size_t)c.extra_slots[2 * t + 0] * kJointExtraDoubles, sum_a);
    store_extra_sum(c.joint_extra + (size_t)c.extra_slots[2 * t + 1] * kJointExtraDoubles, sum_b);
}

// The one choice of the pair-solve kernels' form: launch(G, MATERIALS) with G = lanes per body as std::integral_constant --
// kMaxManifoldPoints up to kSmallWorld bodies, else 1 -- and MATERIALS as std::bool_constant (contact materials: uniform
// over the launch, see pair_solve_derive_body).
template <class Launch>
void with_pair_solve_form(const BodyArrays &b, const ContactBuffers &c, Launch &&launch)
{
    with_flag(c.friction != nullptr, [&](auto materials) {
        if (b.n <= kSmallWorld)
            launch(std::integral_constant<uint32_t, kMaxManifoldPoints>{}, materials);
        else
            launch(std::integral_constant<uint32_t, 1>{}, materials);
    });
}

} // namespace

// ---------------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------------
hipError_t launch_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                   uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row, hipStream_t stream,
                                   const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    const size_t lds_bytes = shape_lds_bytes(s);
    with_flag(trace_masks != nullptr, [&](auto trace) {
        with_flag(c.friction != nullptr, [&](auto materials) {
            with_flag(c.terrain.planes != nullptr, [&](auto terrain) {
                hipLaunchKernelGGL((k_integrate_ground<decltype(trace)::value, decltype(materials)::value, decltype(terrain)::value>),
                                   dim3(blocks_for(items)), dim3(kBlock), lds_bytes, stream, b, s, h, c, subset, last_mask, trace_masks, trace_row);
            });
        });
    });
    return hipGetLastError();
}

hipError_t launch_sat_contact_pairs(const BodyArrays &b, const PolytopeTables &t, const ContactBuffers &c,
                                    uint32_t n_pairs, SatScratch *list, hipStream_t stream, bool dense)
{
    return launch_sat_contacts(b, t, c.rec, c.pairs, n_pairs, c.manifolds, c.pair_codes, list, stream, dense);
}

hipError_t launch_pair_solve_derive(const BodyArrays &b, double *dyn_out, double h, const ContactBuffers &c,
                                    hipStream_t stream, const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    with_pair_solve_form(b, c, [&](auto lanes, auto materials) {
        constexpr uint32_t G = decltype(lanes)::value;
        hipLaunchKernelGGL((k_pair_solve_derive<G, decltype(materials)::value>), dim3(blocks_for(items * G)), dim3(kBlock), 0, stream, b,
                           dyn_out, h, c, subset);
    });
    return hipGetLastError();
}

hipError_t launch_joint_extras(double h, const ContactBuffers &c, hipStream_t stream)
{
    if (!c.joint_extra || c.n_extra_joints == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_joint_extras, dim3(blocks_for(c.n_extra_joints)), dim3(kBlock), 0, stream, h, c);
    return hipGetLastError();
}

hipError_t launch_pair_solve_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                              double *next_rec, uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row,
                                              hipStream_t stream, const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    const size_t lds_bytes = shape_lds_bytes(s);
    with_pair_solve_form(b, c, [&](auto lanes, auto materials) {
        with_flag(trace_masks != nullptr, [&](auto trace) {
            constexpr uint32_t G = decltype(lanes)::value;
            hipLaunchKernelGGL((k_pair_solve_integrate_ground<decltype(trace)::value, G, decltype(materials)::value>), dim3(blocks_for(items * G)),
                               dim3(kBlock), lds_bytes, stream, b, s, h, c, subset, next_rec, last_mask, trace_masks, trace_row);
        });
    });
    return hipGetLastError();
}

hipError_t launch_body_frames_aos(const BodyArrays &b, double *frames, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_body_frames_aos, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, frames);
    return hipGetLastError();
}

hipError_t launch_body_frames(const BodyArrays &b, double *rec, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_body_frames, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, rec);
    return hipGetLastError();
}

hipError_t launch_stat_records(const BodyArrays &b, double *stat_rec, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_stat_records, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, stat_rec);
    return hipGetLastError();
}

} // namespace xpbd
