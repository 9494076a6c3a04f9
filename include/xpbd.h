/*
 * xpbd.h -- C ABI of the MI355X-native XPBD rigid-body stepper.
 *
 * This is the drop-in boundary for the per-substep hot path of
 * jim-ec/constraint_solver: everything below `solver::step`
 * (reference src/solver.rs:3-17) runs in hand-written HIP kernels for gfx950;
 * everything above it (World, Rigid, Polytope construction, the app) stays on
 * the host and calls these entry points.  Plain pointers and sizes only.
 *
 * Reference interface each entry point replaces:
 *   xpbd_step_one               solver::step(&mut Rigid,&Polytope,dt,n)   src/solver.rs:3
 *   xpbd_world_step             World::integrate's loop of solver::step    src/world.rs:34-43
 *   xpbd_world_upload_bodies    the `&mut Rigid` borrows of that loop      src/world.rs:41-42, src/rigid.rs:6-50
 *   xpbd_world_set_shapes       the `&Polytope` borrow (vertices only)     src/solver.rs:3, src/geometry.rs:82-93
 *   xpbd_world_download_bodies  Rigid read-back (frame() for rendering)    src/app.rs:227-230, src/rigid.rs:75-80
 *   xpbd_world_download_contacts  the Vec<Constraint> push order of ground src/collision.rs:16-32
 *
 * Semantics: for every body i,  xpbd_world_step(w, dt, n)  ==
 *   solver::step(&mut body[i], &shape[shape_id[i]], dt, n)
 * in IEEE f64 with the reference's operation order (no FMA contraction), so
 * ground-contact index lists are bit-exact and poses agree with the CPU
 * reference (target 1e-5 relative; observed bit-identical).
 *
 * Threading: one xpbd_world is used from one thread at a time; distinct worlds
 * are independent.  step() enqueues on the world's HIP stream and returns;
 * download_* and synchronize() wait (XPBD_MODE_CONTACTS: step() waits ONCE, for the
 * broadphase's pair counts, which size the pair buffers; everything after that is
 * enqueued).  No call throws or unwinds across the ABI.
 */
#ifndef XPBD_H
#define XPBD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#define XPBD_NOEXCEPT noexcept /* the calls that cannot fail; every other call reports an exception as XPBD_E_OOM */
#else
#define XPBD_NOEXCEPT
#endif

/* 2: xpbd_multi_world_* (library-owned sharding), XPBD_E_HALO, edge_axes_separation, state history */
#define XPBD_ABI_VERSION 2u

/* Error codes (reference has no Result on this path; it panics). */
#define XPBD_OK                   0
#define XPBD_E_INVALID          (-1)  /* bad argument / state */
#define XPBD_E_HIP              (-2)  /* a HIP runtime call failed */
#define XPBD_E_OOM              (-3)  /* host or device allocation failed, or a host thread could not be started */
#define XPBD_E_SINGULAR_INERTIA (-4)  /* mirrors the panic at src/rigid.rs:59 */
#define XPBD_E_NO_DEVICE        (-5)  /* no usable gfx950 device */
#define XPBD_E_CAPACITY         (-6)  /* caller buffer too small */
#define XPBD_E_HALO              (-7)  /* multi-GPU: a body outran halo_margin since the halos were planned */

/* A shape may have at most this many vertices (contact set is a u32 mask). */
#define XPBD_MAX_SHAPE_VERTS 32u

/*
 * repr(C) mirror of the reference's `Rigid` (src/rigid.rs:6-50), field order
 * kept, `color` dropped: 38 doubles = 304 bytes.
 *   inverse_inertia : cgmath Matrix3, column-major, [3*col + row]
 *   rotation        : cgmath Quaternion::new(w, xi, yj, zk) order: {s, x, y, z}
 */
typedef struct xpbd_rigid {
    double inverse_mass;
    double inverse_inertia[9];
    double external_force[3];
    double internal_force[3];
    double external_torque[3];
    double internal_torque[3];
    double velocity[3];
    double angular_velocity[3];
    double center_of_mass[3];
    double position[3];
    double rotation[4];
} xpbd_rigid;

/* One ground constraint of the last substep: body index and the index of the
 * shape vertex that produced it (src/collision.rs:16-32 push order). */
typedef struct xpbd_contact {
    uint32_t body;
    uint32_t vertex;
} xpbd_contact;

/* How xpbd_world_step schedules the substep loop. */
#define XPBD_MODE_FUSED        0u /* one launch runs all substeps in registers (bodies are independent) */
#define XPBD_MODE_PER_SUBSTEP  1u /* one launch per substep: state round-trips HBM each substep */
#define XPBD_MODE_CONTACTS     2u /* EXTENSION: ground + body-body contacts (needs xpbd_world_set_polytopes) */

#define XPBD_FLAG_TRACE_CONTACTS 1u /* keep the contact mask of every substep of the last step() call */

typedef struct xpbd_config {
    uint32_t struct_size;  /* = sizeof(xpbd_config) */
    int32_t  device;       /* HIP device ordinal */
    uint32_t mode;         /* XPBD_MODE_* */
    uint32_t flags;        /* XPBD_FLAG_* */
    uint32_t block_size;   /* threads per workgroup, multiple of 64, <= 256; 0 = library default (64) */
    uint32_t reserved[3];  /* must be 0 */
} xpbd_config;

typedef struct xpbd_world xpbd_world;

/* Library / error ---------------------------------------------------------- */
uint32_t    xpbd_abi_version(void) XPBD_NOEXCEPT;
/* Message for the last failing call on this thread; valid until the next call. */
const char *xpbd_last_error(void) XPBD_NOEXCEPT;
/* Fills cfg with defaults (device 0, fused mode, no flags). */
void        xpbd_config_default(xpbd_config *cfg) XPBD_NOEXCEPT;
/* Number of visible HIP devices, or a negative error code. */
int         xpbd_device_count(void);

/* World lifetime ----------------------------------------------------------- */
int  xpbd_world_create(xpbd_world **out, const xpbd_config *cfg);
void xpbd_world_destroy(xpbd_world *w) XPBD_NOEXCEPT;

/* Shapes: all shapes' vertices back to back (xyz triples) and a CSR offset
 * array of n_shapes+1 entries (in vertices).  Copied; caller keeps ownership.
 * While bodies are resident the new table must still cover every shape id they use (else XPBD_E_INVALID). */
int  xpbd_world_set_shapes(xpbd_world *w, const double *verts_xyz,
                           const uint32_t *vert_offsets, uint32_t n_shapes);

/* Bodies: AoS host array -> SoA device layout.  shape_id may be NULL (all 0). */
int  xpbd_world_upload_bodies(xpbd_world *w, const xpbd_rigid *aos,
                              const uint32_t *shape_id, uint32_t n);
int  xpbd_world_download_bodies(xpbd_world *w, xpbd_rigid *aos, uint32_t n);
uint32_t xpbd_world_body_count(const xpbd_world *w) XPBD_NOEXCEPT;
/* Rigid::frame() of every body (src/rigid.rs:75-80), the only thing the reference's renderer reads per
 * frame (src/app.rs:227-230): frames[7*i .. 7*i+6] = origin x y z, rotation s x y z.  56 B/body instead of 304. */
int  xpbd_world_download_frames(xpbd_world *w, double *frames, uint32_t n);

/* for each body: solver::step(body, shape[body], dt, substeps).  Asynchronous. */
int  xpbd_world_step(xpbd_world *w, double dt, uint32_t substeps);
int  xpbd_world_synchronize(xpbd_world *w);

/* Contacts of the LAST substep of the last step(), sorted by body then vertex
 * (= reference push order).  *n_out receives the total count even when it
 * exceeds cap (then XPBD_E_CAPACITY is returned and out holds the first cap). */
int  xpbd_world_download_contacts(xpbd_world *w, xpbd_contact *out, uint32_t cap,
                                  uint32_t *n_out);
/* With XPBD_FLAG_TRACE_CONTACTS: masks[k*n + i] = bit set of shape vertices of
 * body i that produced a constraint in substep k of the last step() call. */
int  xpbd_world_download_contact_masks(xpbd_world *w, uint32_t *masks,
                                       uint32_t substeps, uint32_t n);

/* Stream interop: run on a caller-owned hipStream_t (NULL restores the
 * world's own stream).  The caller keeps the stream alive. */
int  xpbd_world_set_stream(xpbd_world *w, void *hip_stream);
void *xpbd_world_get_stream(const xpbd_world *w) XPBD_NOEXCEPT;
int  xpbd_world_set_mode(xpbd_world *w, uint32_t mode);

/* Literal single-body drop-in for solver::step (src/solver.rs:3): uploads,
 * steps on device 0 and downloads one body.  verts: nverts xyz triples. */
int  xpbd_step_one(xpbd_rigid *rigid, const double *verts_xyz, uint32_t nverts,
                   double dt, uint32_t substeps);

/* ---------------------------------------------------------------------------
 * EXTENSION -- body-body contacts.  NOT in the reference:
 * its `sat` (src/collision.rs:37-121) is an uncalled stub and `World` holds two
 * bodies that never interact.  These entry points finish that sketch; parity
 * for them is unpinned (own CPU oracle + invariants), and nothing above
 * changes behaviour when they are not used.
 * ------------------------------------------------------------------------- */

/* Full convex polytope (reference `Polytope`, src/geometry.rs:82-93): vertices,
 * edges (vertex index pairs), faces as CSR (face_offsets has n_faces+1 entries
 * into face_indices) and the centroid.  Faces need 3..8 vertices. */
typedef struct xpbd_polytope {
    const double   *vertices_xyz;
    const uint32_t *edges;
    const uint32_t *face_offsets;
    const uint32_t *face_indices;
    uint32_t n_vertices, n_edges, n_faces, reserved;
    double   centroid[3];
} xpbd_polytope;

#define XPBD_MAX_MANIFOLD_POINTS 8u
#define XPBD_FEATURE_FACE_A 0u  /* reference face on A, incident body B */
#define XPBD_FEATURE_FACE_B 1u  /* reference face on B, incident body A */
#define XPBD_FEATURE_EDGES  2u  /* edge of A (reference) against edge of B */

/* Contact manifold of one pair.  p_ref[k] lies on the reference body's surface,
 * p_inc[k] is the penetrating point of the incident body (world space). */
typedef struct xpbd_manifold {
    uint32_t n_points;   /* 0: separated */
    uint32_t feature;    /* XPBD_FEATURE_* (valid when n_points > 0) */
    uint32_t index_a;    /* face of A (reference or incident) or edge of A */
    uint32_t index_b;    /* face of B (incident or reference) or edge of B */
    double   separation; /* largest separating-axis value, < 0 */
    double   p_ref[XPBD_MAX_MANIFOLD_POINTS][3];
    double   p_inc[XPBD_MAX_MANIFOLD_POINTS][3];
} xpbd_manifold;

/* Replaces xpbd_world_set_shapes when body-body contacts are wanted: sets the
 * vertex tables AND the face/edge topology (outward face planes are derived as
 * Polytope::plane does, src/geometry.rs:262-271). */
int  xpbd_world_set_polytopes(xpbd_world *w, const xpbd_polytope *shapes, uint32_t n_shapes);

/* SAT narrowphase of the given body pairs (pairs[2k], pairs[2k+1] = A, B) at the
 * world's current poses: a group of 16, 32 or 64 lanes per pair (by the largest shape).
 * out has n_pairs entries. */
int  xpbd_world_narrowphase(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs,
                            xpbd_manifold *out);

/* The reference's edge_axes_separation (src/collision.rs:151-197: written, but called by nobody there, not even by `sat`)
 * for the given pairs at the world's current poses, literally: all E_A x E_B edge pairs, axis = normalize(eA x eB) turned
 * away from A's centroid, skipped when A has a vertex beyond the edge's foot, distance of B's support along -axis; first
 * maximum wins, parallel edges (NaN axis) contribute nothing.  Returns (f64::MIN, (usize::MAX, usize::MAX)) as
 * (-DBL_MAX, 0xFFFFFFFF, 0xFFFFFFFF).  Diagnostic: the contact pipeline's SAT tests the unique edge DIRECTIONS instead. */
typedef struct xpbd_edge_query {
    double   separation;
    uint32_t edge_a, edge_b;
} xpbd_edge_query;
int  xpbd_world_edge_axes_separation(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_edge_query *out);

/* GJK + EPA narrowphase of the given pairs (the reference has neither): boolean GJK on the
 * Minkowski difference built with the reference's support convention (src/geometry.rs:274-289), then EPA for the
 * penetration depth, the normal (from A to B) and one witness point on each body.  16 or 32 lanes per pair
 * for the boolean GJK, one wave per penetrating pair for EPA. */
#define XPBD_GJK_SEPARATED   0
#define XPBD_GJK_PENETRATING 1
#define XPBD_GJK_DEGENERATE  2  /* origin on the simplex boundary / flat simplex / iteration cap: use the SAT */
typedef struct xpbd_gjk_result {
    int32_t  status;
    uint32_t gjk_iterations, epa_iterations, reserved;
    double   depth;
    double   normal[3];
    double   point_a[3];
    double   point_b[3];   /* point_a - point_b = depth * normal */
} xpbd_gjk_result;
int  xpbd_world_narrowphase_gjk(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_gjk_result *out);
/* Narrowphase used by XPBD_MODE_CONTACTS: the SAT (default: up to 8 points per pair) or GJK + EPA (a clipped face
 * contact where the penetration normal is a face normal of one of the bodies, else one point with reference body A /
 * incident body B; a degenerate query gives no contact in that substep).  In the pipeline a pair that GJK finds
 * separated keeps the direction that proved it, and the pair's next query within the same step call tries that
 * support plane first (a settled pile: most separated pairs stay separated by the same plane). */
#define XPBD_NARROWPHASE_SAT     0u
#define XPBD_NARROWPHASE_GJK_EPA 1u
int  xpbd_world_set_narrowphase(xpbd_world *w, uint32_t narrowphase);
/* In XPBD_MODE_CONTACTS both narrowphases first test the TIGHT bounding spheres of a pair (centroid, largest
 * vertex distance): the neighbour lists are built once per step call from spheres inflated by a whole frame of
 * travel, so in a given substep most pairs of a loose scene cannot touch, and those are answered "no contact"
 * without running the query.  (xpbd_world_narrowphase / _gjk, the diagnostic entry points, always run it.)
 * For the SAT the test can run inside the narrowphase kernel (ONE_PASS) or as a pass of its own followed by the SAT
 * over the surviving pairs only (TWO_PASS; that pass also answers the pairs still separated by the face axis that
 * separated them last time -- the SAT's own arithmetic for that face): identical results, different cost -- AUTO
 * picks per step call from the share of touching pairs in the previous one.  GJK + EPA always runs it as a pass. */
#define XPBD_SAT_SCHEDULE_AUTO     0u
#define XPBD_SAT_SCHEDULE_ONE_PASS 1u
#define XPBD_SAT_SCHEDULE_TWO_PASS 2u
int  xpbd_world_set_sat_schedule(xpbd_world *w, uint32_t schedule);

/* XPBD_MODE_CONTACTS: per xpbd_world_step a sphere broadphase builds sorted neighbour lists
 * (sphere = centroid, r_shape + min(|v| dt, r_shape) + pad); per substep: integrate -> SAT of every neighbour
 * pair -> ground contacts (reference path) -> pair contacts, Jacobi-averaged with a fixed
 * summation order -> derive.  Exact semantics: oracle/xpbd_pairs_oracle.h.  With no overlapping
 * spheres the result equals XPBD_MODE_PER_SUBSTEP bit for bit. */
int  xpbd_world_set_contact_pad(xpbd_world *w, double pad);            /* default 0.02 (metres) */
/* Optional limit on how fast a BODY-BODY contact may push its bodies apart: the length of a contact point's positional
 * correction is limited to max(0, speed * h - what the incident point has already moved towards the reference surface in
 * this substep) before lambda is formed, so the bodies part at `speed` instead of accelerating (0 = off, the default = the reference's solver loop,
 * src/solver.rs:19-27, which resolves any penetration within ONE substep, i.e. at depth / h -- 120 m/s for 0.1 m at 20
 * substeps per frame; light bodies squeezed between heavy ones leave a pile at that speed).  With the knob on, the ground
 * contacts of XPBD_MODE_CONTACTS are limited the same way; joints never are; XPBD_MODE_FUSED / _PER_SUBSTEP (the reference path)
 * ignore it.  Semantics: oracle/xpbd_pairs_oracle.h. */
int  xpbd_world_set_max_depenetration_speed(xpbd_world *w, double speed);
/* out = {neighbour pairs of the last step, touching pairs, manifold points}; the last two are
 * summed over substeps since the previous call and then reset. */
int  xpbd_world_contact_stats(xpbd_world *w, uint64_t out[3]);
/* Broadphase alone (as the next step(dt, .) would run it) and its CSR neighbour lists. */
int  xpbd_world_build_neighbours(xpbd_world *w, double dt, uint32_t *n_entries_out);
int  xpbd_world_download_neighbours(xpbd_world *w, uint32_t *offsets, uint32_t *neighbours, uint32_t cap);

/* Joints (EXTENSION; the reference has no joint type, only the unused `distance`
 * field of Constraint, src/constraint.rs:9).  A joint keeps |frame_b * anchor_b - frame_a * anchor_a|
 * at `distance` (anchors in object space, the space of the shape vertices).  distance = 0 is a ball
 * joint; XPBD_JOINT_HINGE adds an angular term (below).  Joints are projected in XPBD_MODE_CONTACTS together
 * with the body-body contacts (same Jacobi pass, after a body's contacts, ascending joint index).
 * Body indices refer to the bodies uploaded last; uploading bodies again clears the joints.
 * Only XPBD_MODE_CONTACTS projects joints: in the other modes a non-empty list is XPBD_E_INVALID.
 * After a failed call (XPBD_E_OOM, XPBD_E_HIP) the previous joints, limits and drives are all still in force. */
#define XPBD_JOINT_DISTANCE 0u  /* positional term only (distance = 0: ball joint) */
/* (XPBD_JOINT_SLIDER = 2: see "SLIDERS and joint DRIVES" below) */
#define XPBD_JOINT_HINGE    1u  /* positional term + ANGULAR term: the unit axes axis_a / axis_b (object space of a / b) are kept
                                 * aligned.  With a_w = rot_a * axis_a, b_w = rot_b * axis_b: delta = a_w x b_w, n = delta / |delta|,
                                 * w = sum over both bodies of (I^-1 (q^-1 n)) . (q^-1 n) (the angular half of
                                 * Constraint::inverse_resitance, src/constraint.rs:25-32), lambda = |delta| / (w + compliance);
                                 * a turns by +lambda n, b by -lambda n, applied as Rigid::apply_impulse applies an angular
                                 * displacement (src/rigid.rs:118-122).  It is a Jacobi entry of its own, after the joint's
                                 * positional term.  A hinge = ball joint (distance 0) on the axis + this: one degree of freedom. */
typedef struct xpbd_joint {
    uint32_t body_a, body_b;
    double   anchor_a[3];
    double   anchor_b[3];
    double   distance;
    double   axis_a[3];   /* XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER: unit vectors */
    double   axis_b[3];
    uint32_t kind;        /* XPBD_JOINT_* */
    uint32_t reserved;    /* must be 0 */
} xpbd_joint;
int  xpbd_world_set_joints(xpbd_world *w, const xpbd_joint *joints, uint32_t n_joints);

/* Angular joint LIMITS (EXTENSION; Mueller et al. 2020, "Detailed Rigid Body Simulation with Extended Position Based
 * Dynamics", 3.3): a stop on the rotation a joint leaves free.  With q_a, q_b the body rotations, a_w = q_a * axis_a,
 * b_w = q_b * axis_b, r_a = q_a * ref_a, r_b = q_b * ref_b, every limit measures an angle phi about an axis n:
 *   XPBD_LIMIT_HINGE  n = a_w;  phi = atan2((r_a x r_b) . n, r_a . r_b)
 *   XPBD_LIMIT_SWING  c = a_w x b_w;  phi = atan2(|c|, a_w . b_w);  n = c / |c|  (|c| = 0: no entry)
 *   XPBD_LIMIT_TWIST  n = (a_w + b_w) / |a_w + b_w|  (length 0: no entry);  p_a, p_b = r_a, r_b without their components
 *                     along n;  phi = atan2((p_a x p_b) . n, p_a . p_b)
 * err = phi - clamp(phi, lower, upper).  err == 0: the limit adds nothing (no Jacobi entry, the count is unchanged), so a
 * world whose limits never bind steps bit for bit as the same world without them.  Otherwise
 * w = sum over both bodies of (I^-1 (q^-1 n)) . (q^-1 n), lambda = err / (w + compliance), and a turns by +lambda n, b by
 * -lambda n, applied as the hinge's angular term applies its turn.  Every active limit is one Jacobi entry, after its
 * joint's positional and hinge terms, in the order the caller listed the joint's limits.
 * phi is computed with the device's f64 atan2, which is not correctly rounded: results are bit-identical from run to run
 * and between a sharded and a single world, not against a CPU model (which agrees to rounding).
 * Limits name joints of the last xpbd_world_set_joints; setting joints or uploading bodies clears them; n_limits = 0 clears
 * them.  XPBD_E_INVALID (the previous limits stay in place): a world not in XPBD_MODE_CONTACTS, a joint index out of range,
 * a kind that does not fit the joint (HINGE needs XPBD_JOINT_HINGE, SWING and TWIST need XPBD_JOINT_DISTANCE with unit
 * axis_a / axis_b), two limits of one kind on one joint, a non-unit ref_a / ref_b or one not perpendicular to its axis
 * (HINGE, TWIST; |ref|^2 and ref . axis within 1e-3 as the hinge's axes), NaN bounds, bounds outside
 * -pi <= lower <= upper <= pi, SWING with lower != 0.  After a failed call (XPBD_E_OOM, XPBD_E_HIP) the previous limits
 * are still in force, as are the joints and the drives. */
#define XPBD_LIMIT_HINGE 0u  /* joint kind HINGE: signed angle about a_w from r_a to r_b in [lower, upper] */
#define XPBD_LIMIT_SWING 1u  /* joint kind DISTANCE: angle between a_w and b_w <= upper (lower must be 0) */
#define XPBD_LIMIT_TWIST 2u  /* joint kind DISTANCE: signed twist about the bisector of a_w, b_w in [lower, upper] */
typedef struct xpbd_joint_limit {
    uint32_t joint;          /* index into the list of the last xpbd_world_set_joints */
    uint32_t kind;           /* XPBD_LIMIT_* */
    double   ref_a[3];       /* HINGE, TWIST: unit vector perpendicular to axis_a, object space of body_a */
    double   ref_b[3];       /* HINGE, TWIST: unit vector perpendicular to axis_b, object space of body_b */
    double   lower, upper;   /* radians */
} xpbd_joint_limit;          /* 72 bytes */
int  xpbd_world_set_joint_limits(xpbd_world *w, const xpbd_joint_limit *limits, uint32_t n_limits);

/* SLIDERS and joint DRIVES (EXTENSION): a joint that lets a body translate along a line, and joints that do work.
 *
 * XPBD_JOINT_SLIDER (a kind of xpbd_joint) is a cylindrical joint: body b's anchor may move along body a's axis and the two
 * axes stay aligned.  It needs unit axis_a / axis_b (the hinge's tolerance) and distance == 0.  It has the hinge's angular
 * term but NOT the positional term; its anchor is held by the perpendicular term below.  Wherever a HINGE joint is accepted
 * (XPBD_LIMIT_HINGE) a SLIDER is too: a prismatic joint is a slider with an XPBD_LIMIT_HINGE of lower = upper = 0.
 * XPBD_LIMIT_SLIDE (a kind of xpbd_joint_limit, SLIDER joints only) bounds the travel: lower <= upper, both finite, in
 * metres (the [-pi, pi] rule is for the angular kinds); ref_a / ref_b are ignored; at most one per joint.
 * An xpbd_joint_drive moves the degree of freedom a joint leaves free.  compliance alpha >= 0 and finite (0: as stiff as
 * a limit; rad/(N m) or m/N); max_force > 0, +inf allowed (N m or N).
 *
 * Every term is evaluated at the poses the joint pass sees, with c = 1e-6 / h^2, p_a, p_b the world anchors, d = p_b - p_a,
 * a_w = q_a * axis_a, s = d . a_w, W(body, p, n) = Constraint::inverse_resitance (as the positional term), Wang(n) the
 * angular w of the limits; a subscript 0 is the same expression at the poses of the START of the substep.  A joint's extra
 * entries, in this order, are summed among themselves from 0 (position, rotation, count) and the sum is added to each
 * body's accumulator after the joint's positional, hinge and angular-limit entries, only when its count is nonzero:
 *   1. SLIDER, perpendicular term: r = d - a_w s, len = |r| (0: no entry), n = r / len, lambda = len / (W_a(p_a, n) +
 *      W_b(p_b, n) + c); a gets the impulse +lambda n at p_a, b gets -lambda n at p_b, as the positional term applies its own.
 *   2. XPBD_LIMIT_SLIDE: e = s - clamp(s, lower, upper) (0: no entry), n = a_w, lambda = e / (W_a + W_b + c), applied as 1.
 *   3. the drives, in the caller's order.  n = a_w.  With phi the angle of XPBD_LIMIT_HINGE (from ref_a, ref_b) and
 *      wrap(x) = x > pi ? x - 2 pi : (x < -pi ? x + 2 pi : x):
 *        ANGLE             e = wrap(phi - target)                  ANGULAR_VELOCITY  e = wrap(phi - phi_0) - target h
 *        POSITION          e = s - target                          VELOCITY          e = (s - s_0) - target h
 *      e == 0: no entry.  w = Wang(n) (angular kinds: a turns by +lambda n, b by -lambda n, as a limit does) or W_a + W_b
 *      (linear kinds: applied as 2);  lambda = e / (w + (1e-6 + alpha) / h^2), then clamped to +-max_force h^2.  The entry
 *      counts even when lambda was clamped.
 * The velocity drives keep no state: they ask for target * h of motion within every substep, so history restore reproduces
 * a run bit for bit and a sharded world equals the single one.  A world without sliders, SLIDE limits and drives steps bit
 * for bit as before.
 * Drives name joints of the last xpbd_world_set_joints; setting joints or uploading bodies clears them; n_drives = 0 clears
 * them; xpbd_world_set_joint_limits and xpbd_world_set_joint_drives do not clear each other.  XPBD_E_INVALID (the previous
 * drives stay in place): a world not in XPBD_MODE_CONTACTS, a joint index out of range, an unknown kind, a kind that does
 * not fit the joint, two angular or two linear drives on one joint, a non-unit ref_a / ref_b or one not perpendicular to its
 * axis (angular kinds; the limits' 1e-3 tolerances), a non-finite target, an ANGLE target outside [-pi, pi], a negative or
 * non-finite compliance, a max_force that is <= 0 or NaN.  After a failed call (XPBD_E_OOM, XPBD_E_HIP) the previous drives
 * are still in force, as are the joints and the limits. */
#define XPBD_JOINT_SLIDER 2u              /* xpbd_joint.kind */
#define XPBD_LIMIT_SLIDE 3u               /* xpbd_joint_limit.kind: joint kind SLIDER, s in [lower, upper] metres */
#define XPBD_DRIVE_ANGLE 0u               /* joint kind HINGE or SLIDER: phi -> target (rad); refs as XPBD_LIMIT_HINGE */
#define XPBD_DRIVE_ANGULAR_VELOCITY 1u    /* joint kind HINGE or SLIDER: phi moves by target (rad/s) * h per substep; refs as above */
#define XPBD_DRIVE_POSITION 2u            /* joint kind SLIDER: s -> target (m) */
#define XPBD_DRIVE_VELOCITY 3u            /* joint kind SLIDER: s moves by target (m/s) * h per substep */
typedef struct xpbd_joint_drive {
    uint32_t joint;          /* index into the list of the last xpbd_world_set_joints */
    uint32_t kind;           /* XPBD_DRIVE_* */
    double   ref_a[3];       /* angular kinds: unit vector perpendicular to axis_a, object space of body_a */
    double   ref_b[3];       /* angular kinds: unit vector perpendicular to axis_b, object space of body_b */
    double   target;         /* rad, rad/s, m, m/s */
    double   compliance;     /* alpha */
    double   max_force;      /* N m or N */
} xpbd_joint_drive;          /* 80 bytes */
int  xpbd_world_set_joint_drives(xpbd_world *w, const xpbd_joint_drive *drives, uint32_t n_drives);

/* Joint STATES and drive TARGETS (EXTENSION): an encoder on every joint, and a control input that stays on the device.
 *
 * xpbd_world_joint_states evaluates, for the listed joints (joints == NULL: all of them, n = the joint count), the quantities
 * the joint pass works with, at the poses xpbd_world_download_bodies would return at that point of the world's stream.  The
 * symbols are those of the sections above: p_a, p_b the world anchors, d = p_b - p_a, a_w = q_a * axis_a, b_w = q_b * axis_b,
 * s = d . a_w; the velocity of a point p of a body is v_p = velocity + angular_velocity x (p - (position + center_of_mass)),
 * angular_velocity (omega) in world space, as derive leaves it.  Every expression is the solver's own, in its order, so a bound
 * that the report calls violated is one the next substep would act on at these poses.
 *   angle, angle_rate  HINGE and SLIDER joints that have references: those of the joint's angular drive if it has one
 *                      (XPBD_JOINT_STATE_ANGLE_OF_DRIVE), otherwise those of its XPBD_LIMIT_HINGE; with neither the angle is
 *                      not available.  The idiom for a free hinge: an XPBD_LIMIT_HINGE of [-pi, pi] never binds, leaves the
 *                      step bit for bit unchanged, and gives the hinge an encoder.  The angle is in [-pi, pi]; turns are not counted.
 *   flags              which fields are available (a field that is not is +0.0 with its flag clear), and the status of the
 *                      joint's limits by the very comparisons the solver uses (phi < lower, phi > upper; s likewise),
 *                      always with the limit's own references, even where `angle` is reported with the drive's.
 * The call reads only and wakes nobody; it is accepted in every mode, and a world without joints accepts n == 0.
 * The host variant waits.  XPBD_E_INVALID, with nothing written: a NULL world, a NULL out with n > 0, joints == NULL with n
 * other than the joint count, an index out of range.  The device variant enqueues on the world's stream and waits for nothing
 * (dev_out: 16-byte aligned); for an index out of range it writes a record with kind = 0xFFFFFFFF and everything else zero.
 *
 * xpbd_world_set_drive_targets replaces the `target` of resident drives and nothing else: kind, references, compliance and
 * max_force stay, and the next substep that runs sees the new target exactly as if xpbd_world_set_joint_drives had been given
 * the whole table with it.  drives[k] indexes the list of the last xpbd_world_set_joint_drives (NULL: all of them, n = the
 * drive count); the indices must be strictly ascending.  The host variant applies that call's target rules and waits:
 * XPBD_E_INVALID, with nothing changed, for a NULL world, NULL targets with n > 0, drives == NULL with n other than the drive
 * count, an index out of range or not above its predecessor, a non-finite target, an ANGLE target outside [-pi, pi].  The
 * device variant only enqueues; an entry that breaks one of those rules is skipped (entry k is compared with dev_drives[k - 1]
 * whether or not that one was valid, so which entries count does not depend on the schedule; a list that names a drive again
 * after a descent can leave two valid entries for it, and which of their targets it keeps is then unspecified).
 * With sleeping on, both variants request a wake for the groups of the asleep ends of the named drives' joints, as an edit of
 * those bodies would; a fixed end requests nothing (the anchor did not move) and nobody else wakes --
 * xpbd_world_set_joint_drives wakes every body.  xpbd_world_set_joint_limits and the population changes keep the targets set
 * here.  History push and restore do not carry targets, as they do not carry drives.
 * Not here: the multi-GPU world; editing compliance or max_force in place; multi-turn angle counting; joint reactions (the
 * impulse a joint applies differs at its two ends under the Jacobi averaging, and is not reported). */
#define XPBD_JOINT_STATE_HAS_ANGLE       0x001u
#define XPBD_JOINT_STATE_HAS_TRAVEL      0x002u
#define XPBD_JOINT_STATE_HAS_SWING       0x004u
#define XPBD_JOINT_STATE_HAS_TWIST       0x008u
#define XPBD_JOINT_STATE_ANGLE_OF_DRIVE  0x010u  /* angle, angle_rate use the angular drive's references */
#define XPBD_JOINT_STATE_ANGLE_BELOW     0x100u  /* XPBD_LIMIT_HINGE: phi < lower */
#define XPBD_JOINT_STATE_ANGLE_ABOVE     0x200u  /*                   phi > upper */
#define XPBD_JOINT_STATE_TRAVEL_BELOW    0x400u  /* XPBD_LIMIT_SLIDE: s < lower */
#define XPBD_JOINT_STATE_TRAVEL_ABOVE    0x800u  /*                   s > upper */
#define XPBD_JOINT_STATE_SWING_ABOVE     0x1000u /* XPBD_LIMIT_SWING: phi > upper */
#define XPBD_JOINT_STATE_TWIST_BELOW     0x2000u /* XPBD_LIMIT_TWIST: phi < lower */
#define XPBD_JOINT_STATE_TWIST_ABOVE     0x4000u /*                   phi > upper */
#define XPBD_JOINT_STATE_NO_JOINT        0xFFFFFFFFu /* xpbd_joint_state.kind of an index out of range (device variant) */
typedef struct xpbd_joint_state {   /* 80 bytes */
    double   separation;    /* DISTANCE, HINGE: |d| - distance, the positional term's error.  SLIDER: |d - a_w s|, the perpendicular term's len */
    double   misalignment;  /* HINGE, SLIDER: |a_w x b_w|, the angular term's mag.  DISTANCE: +0.0 */
    double   angle;         /* HINGE, SLIDER with references (above): phi of XPBD_LIMIT_HINGE, in [-pi, pi] */
    double   angle_rate;    /* same joints: (omega_b - omega_a) . a_w, rad/s */
    double   travel;        /* SLIDER: s = d . a_w, metres */
    double   travel_rate;   /* SLIDER: (v_pb - v_pa) . a_w + d . (omega_a x a_w), m/s */
    double   swing;         /* DISTANCE with a SWING or TWIST limit: phi of XPBD_LIMIT_SWING */
    double   twist;         /* DISTANCE with a TWIST limit: phi of XPBD_LIMIT_TWIST (|a_w + b_w| = 0: not available) */
    uint32_t joint, kind, flags, reserved;
} xpbd_joint_state;
int  xpbd_world_joint_states(xpbd_world *w, const uint32_t *joints /* NULL: all, n = joint count */, uint32_t n, xpbd_joint_state *out);
int  xpbd_world_joint_states_device(xpbd_world *w, const uint32_t *dev_joints /* NULL: all */, uint32_t n, xpbd_joint_state *dev_out);
int  xpbd_world_set_drive_targets(xpbd_world *w, const uint32_t *drives /* NULL: all, n = drive count */, const double *targets, uint32_t n);
int  xpbd_world_set_drive_targets_device(xpbd_world *w, const uint32_t *dev_drives /* NULL: all */, const double *dev_targets, uint32_t n);

/* KINEMATIC bodies (EXTENSION): fixed bodies that move on a script and push and carry what they meet -- elevators, doors,
 * platforms, conveyors, spinners.
 *
 * A kinematic body is a FIXED body (inverse_mass and all nine inverse_inertia entries == 0, the islands' definition) that has
 * an entry in the world's kinematic table.  Take a frame xpbd_world_step(dt, S), h = dt / S, and substep k = 0..S-1 with
 * r = S - k substeps left.  Before the integrate stage of substep k the two velocities of every entry's body are overwritten
 * from its current position p and rotation q (what xpbd_world_download_bodies would show at that point); all arithmetic per
 * component, no fused multiply-add, correctly rounded divisions:
 *   XPBD_KINEMATIC_POSE      linear = target position p_t, angular = target rotation q_t {s, x, y, z}
 *     velocity = (p_t - p) / ((double)r * h)
 *     dq = q_t * conjugate(q); if dq.s < 0 then dq = -dq;  m = length(vec(dq))
 *     m == 0: angular_velocity = 0;  else half = atan2(m, dq.s), angular_velocity = vec(dq) * ((2 / h) * tan(half / r) / m)
 *     This is the exact inverse of the integrate stage's rotation update, which turns a body by the half angle atan(h |w| / 2)
 *     about w: the body turns half / r per substep and arrives at q_t in the last one.  q_t need not be unit, only the ratio
 *     m : s enters.  The target persists: in later frames p == p_t, the velocities are zero and the body holds.
 *   XPBD_KINEMATIC_VELOCITY  linear = velocity, angular = {wx, wy, wz, ignored}
 *     velocity = linear, angular_velocity = angular[0..2], re-asserted before every substep (a fixed body that was merely given
 *     a velocity through xpbd_world_set_dynamics loses angular speed in every substep: derive recomputes it from the rotation
 *     the body made).  The pose follows the integrate stage: a substep turns the body by 2 atan(h |w| / 2), not by h |w|.
 * After the overwrite everything is what a fixed body with those velocities does: integrate moves it, no constraint moves it
 * (its inverse mass is zero), and derive leaves the velocities its neighbours' restitution pass reads.  The compliance term
 * 1e-6 / h^2 keeps a contact's lagrange finite where both inverse masses are zero, so a kinematic body may cross the ground,
 * the terrain or another fixed body without effect.  The k = 0 overwrite happens before the broadphase, so the bounding spheres
 * of the frame include the scripted travel.
 *
 * xpbd_world_set_kinematics replaces the whole table (n == 0 clears it); `body` strictly ascending.  It reads the ten mass
 * doubles of the named bodies from the device and may wait for that.  XPBD_E_INVALID, with the table as it was: a NULL world,
 * a NULL list with n > 0, no resident bodies, an index out of range or not above its predecessor, an unknown mode, a body that
 * is not fixed, any non-finite value (angular[3] of a VELOCITY entry included), an all-zero POSE rotation.
 * xpbd_world_set_kinematic_targets replaces the seven doubles (linear, angular) of resident entries and nothing else: the mode
 * and the body stay, and the next substep that runs sees the new row exactly as if xpbd_world_set_kinematics had been given the
 * whole table with it.  entries[k] indexes the table of the last xpbd_world_set_kinematics (NULL: all of them, n = the entry
 * count); the indices must be strictly ascending.  The host variant applies that call's value rules and waits: XPBD_E_INVALID,
 * with nothing changed, for a NULL world, NULL rows with n > 0, entries == NULL with n other than the entry count, an index out
 * of range or not above its predecessor, a non-finite value, an all-zero POSE rotation.  The device variant only enqueues
 * (dev_rows 8-byte aligned, n <= 2^29); an entry that breaks one of those rules is skipped (entry k is compared with
 * dev_entries[k - 1] whether or not that one was valid, so which entries count does not depend on the schedule; a list that
 * names an entry again after a descent can leave two valid rows for it, and which of them it keeps is then unspecified).
 * Neither variant wakes anybody by itself (see SLEEPING: a body that MOVES wakes what it meets).
 * xpbd_world_upload_bodies clears the table, as it clears joints and filters.  A population change keeps the entries of the
 * surviving bodies, re-indexed, in order, and drops those of removed bodies; added bodies are not kinematic.  History push and
 * restore do not carry the table, as they do not carry drives; the definition uses no stored start pose, so a run repeated from
 * a restored entry with the same targets gives the same bits.
 * The table is accepted in every mode; only xpbd_world_step in XPBD_MODE_CONTACTS applies it, and a frame with a non-empty
 * table runs the unfused schedule (as restitution and terrain do).  While it is non-empty the split API
 * (xpbd_world_contacts_begin / _substep) is XPBD_E_INVALID.  A world that never calls these, or whose table is empty, launches
 * what it launched before.
 * Not here: the multi-GPU world; a form of the fused schedule that applies the table.  (Making a body with mass kinematic:
 * freeze it first, "MASS properties of resident bodies".) */
#define XPBD_KINEMATIC_POSE     0u  /* linear = target position, angular = target rotation {s,x,y,z} */
#define XPBD_KINEMATIC_VELOCITY 1u  /* linear = velocity, angular = {wx, wy, wz, ignored} */
typedef struct xpbd_kinematic {     /* 64 bytes */
    uint32_t body, mode;
    double   linear[3];
    double   angular[4];
} xpbd_kinematic;
int  xpbd_world_set_kinematics(xpbd_world *w, const xpbd_kinematic *list, uint32_t n);   /* whole table; n == 0 clears */
int  xpbd_world_set_kinematic_targets(xpbd_world *w, const uint32_t *entries /* NULL: all, n = entry count */,
                                      const double *rows /* [n][7] */, uint32_t n);
int  xpbd_world_set_kinematic_targets_device(xpbd_world *w, const uint32_t *dev_entries /* NULL: all */, const double *dev_rows, uint32_t n);
uint32_t xpbd_world_kinematic_count(const xpbd_world *w) XPBD_NOEXCEPT;

/* Collision FILTERS (EXTENSION): which body-body pairs may touch.
 * Pair rule: bodies i and j may touch iff (group_i & mask_j) != 0 && (group_j & mask_i) != 0; with XPBD_FILTER_JOINTED
 * they also may not touch when any joint of the world's current joint list connects them.  The rule is symmetric.
 * Defaults: without filters every body is {~0u, ~0u}.  filters == NULL with n == 0 sets that default (flags may still turn
 * on XPBD_FILTER_JOINTED); otherwise n must equal xpbd_world_body_count (the multi world: n_global), the caller's order.
 * What is filtered: body-body contacts only, in the broadphase.  A filtered pair is absent from the neighbour lists
 * (xpbd_world_download_neighbours), from the pair list and from xpbd_world_contact_stats' pair count.  Ground contacts (the
 * reference path), joints (they still act between filtered bodies) and the plain ray casts (they keep hitting every body)
 * are not affected.  Accepted in every mode; XPBD_MODE_FUSED / _PER_SUBSTEP have no body-body contacts, so there the filters
 * matter only to the masked ray casts.
 * Masked ray casts: a ray can hit body b only if (group_b & mask) != 0; everything else as the ray casts below (nearest hit,
 * ties to the smaller index, ignore_body, same bits on the grid and brute-force paths).
 * Lifetime: xpbd_world_upload_bodies / xpbd_multi_world_upload clear the filters and the flags (as they clear joints);
 * xpbd_world_set_joints leaves them alone (XPBD_FILTER_JOINTED applies to the joints present when the next broadphase runs);
 * history push / restore do not touch them.
 * XPBD_E_INVALID (the previous filters stay in place): a NULL world, filters == NULL with n > 0, filters != NULL with n not
 * equal to the body count, unknown flag bits.  The multi-world call is not collective: every rank passes the same list (as
 * xpbd_multi_world_set_joint_limits); a device failure while the filters are handed to the shards leaves that world unusable.
 * A world without filters, or with all {~0u, ~0u} and flags = 0, steps bit for bit as before. */
#define XPBD_FILTER_JOINTED 1u   /* two bodies joined by a joint of the world never collide */
typedef struct xpbd_collision_filter {   /* 8 bytes */
    uint32_t group;                      /* the layers this body is in */
    uint32_t mask;                       /* the layers it collides with */
} xpbd_collision_filter;
int  xpbd_world_set_collision_filters(xpbd_world *w, const xpbd_collision_filter *filters, uint32_t n, uint32_t flags);

/* Contact MATERIALS (EXTENSION): Coulomb friction at the position level, per body and for the ground plane.
 * Every body has a friction coefficient friction_b and the ground plane has one, ground_friction: doubles >= 0, +inf allowed
 * and the default.  The coefficient of a contact is the smaller of its two sides' (exact, symmetric, no inf * 0):
 *   mu = min(friction_inc, friction_ref)      for a body-body contact point,
 *   mu = min(friction_b, ground_friction)     for a ground contact.
 * Both contact kinds form `correction` (ground: target - x; pair: p_ref - p_inc) and `delta_tangential`, the tangential part
 * of the contact point's (relative) motion during the substep.  The reference subtracts all of it from the contact's target
 * (collision::ground: `target_position - 1.0 * delta_tangential_position`); with materials the literal 1.0 becomes k:
 *   len_c = length(correction), len_t = length(delta_tangential)       (sqrt(dot(..)), as everywhere else)
 *   bound = mu * len_c
 *   k     = (bound < len_t) ? bound / len_t : 1.0
 *   c1    = (target | p_ref) - k * delta_tangential
 * and everything after c1 (difference, distance, direction, w, the depenetration limit -- whose `closing` uses delta and
 * correction, not c1 --, lambda, the impulses, the Jacobi average) is unchanged.  This is Coulomb's cone on positions: len_c,
 * the penetration the contact removes in this substep, stands for the normal impulse, and the contact may take back at most
 * mu * len_c of the tangential slip; a contact that slips less sticks exactly as without materials (k = 1.0).  The comparison
 * is false for mu = +inf, for len_c = 0 with mu = +inf (bound is NaN), for len_t = 0 and for any NaN: all keep k = 1.0.
 * Hence a world without materials, or with every coefficient +inf, steps bit for bit as before.
 * Where: XPBD_MODE_CONTACTS only, its ground contacts and its pair contacts under both narrowphases.  XPBD_MODE_FUSED /
 * _PER_SUBSTEP (the pinned reference path) accept the call and ignore the values, as they ignore the depenetration limit.
 * Joints, joint limits, filters, ray casts, contact reports (still the manifolds at the post-integrate poses) and history
 * are not affected.
 * Defaults: materials == NULL with n == 0 makes every body +inf (ground_friction still applies); otherwise n must equal
 * xpbd_world_body_count (the multi world: n_global), the caller's order.
 * Lifetime: xpbd_world_upload_bodies / xpbd_multi_world_upload reset every coefficient to +inf; xpbd_world_set_joints,
 * history push / restore and mode changes leave the materials alone.
 * XPBD_E_INVALID (the previous materials stay in place): a NULL world, materials == NULL with n > 0, materials != NULL with n
 * not equal to the body count, a negative or NaN coefficient (ground_friction included), a nonzero `reserved`. */
typedef struct xpbd_material {   /* 16 bytes */
    double friction;             /* >= 0, may be +inf (the default: the reference's contact) */
    double reserved;             /* must be 0 (room for restitution) */
} xpbd_material;
int  xpbd_world_set_materials(xpbd_world *w, const xpbd_material *materials, uint32_t n, double ground_friction);

/* RESTITUTION (EXTENSION): bouncing contacts, a velocity pass after derive.
 * Every body has a restitution coefficient restitution_b and the ground plane has one, ground_restitution: doubles in [0, 1],
 * 0 the default; bounce_threshold >= 0 (m/s, finite, default 0) is the closing speed below which a contact does not bounce.
 * The coefficient of a contact is the larger of its two sides', written as a compare-and-select:
 *   e = (e_inc < e_ref) ? e_ref : e_inc             for a body-body contact point,
 *   e = (e_b < ground_restitution) ? ground_restitution : e_b      for a ground contact.
 * Where: XPBD_MODE_CONTACTS only, as stage 6 of every substep, after Rigid::derive (stage 5 of oracle/xpbd_pairs_oracle.h),
 * under both narrowphases, on the manifolds and the ground contact mask of THIS substep (both formed at the post-integrate
 * poses).  xpbd_world_step and xpbd_world_contacts_substep run it alike.
 * Notation.  v0, w0: a body's velocity and angular velocity at the start of the substep (before integrate); x, q, v, w: its
 * position, rotation and velocities after derive; c = x + center_of_mass.  For a world point p of a body, with arm = p - c:
 *   u(p)  = v  + cross(w,  arm)            u0(p) = v0 + cross(w0, arm)
 *   W(p, n) = inverse_mass + dot(inverse_inertia * a, a),  a = conjugate(q) * cross(arm, n)      (inverse_resistance at x, q)
 * and an impulse P at p changes the body as the position pass applies a correction:
 *   v += P * inverse_mass            w += cross(inverse_inertia * arm, P)
 * dot(a, b) is (a.x * b.x + a.y * b.y) + a.z * b.z and length is sqrt(dot(..)), as everywhere else.
 * Pair contact point, with p_inc and p_ref exactly as the position pass forms them (a face contact: the stored point on the
 * incident body and its projection onto the reference plane; the one-point contact: its two points):
 *   n      = the reference plane's normal (face contact), or d * (1.0 / length(d)) with d = p_ref - p_inc (one-point contact;
 *            no entry when length(d) == 0).  Both point out of the reference body.
 * One MANIFOLD is solved by sequential impulses on copies (v_inc, w_inc, v_ref, w_ref) of its two bodies' post-derive
 * velocities; every point k keeps total_k, the impulse it has applied so far, which starts at 0 and is never negative.
 * XPBD_RESTITUTION_SWEEPS passes over the points in point order; a visit of point k computes, with u taken from the copies as
 * they are at that moment and u0 from v0, w0:
 *   vn     = dot(n, u_inc(p_inc) - u_ref(p_ref))          vn0 = dot(n, u0_inc(p_inc) - u0_ref(p_ref))
 *   Wsum   = W_inc(p_inc, n) + W_ref(p_ref, n)
 *   the visit does nothing unless  e > 0 && vn0 < -bounce_threshold && Wsum > 0  (two immovable bodies: never);
 *   wanted = total_k + ((-e) * vn0 - vn) / Wsum           (no compliance);   if (!(wanted > 0)) wanted = 0
 *   lambda = wanted - total_k;   nothing more when lambda == 0;   total_k = wanted
 *   P = lambda * n on the incident copy at p_inc, (-lambda) * n on the reference copy at p_ref, applied at once.
 * So a point pushes (lambda > 0) while it closes faster than (-e) * vn0 allows and gives back (lambda < 0) at most what it has
 * pushed: the manifold converges to the impulses that make every pushing point leave at exactly e times its closing speed.
 * (An average over the points, as the position pass forms it, delivers a quarter of a four-point face contact per substep and
 * never reaches e; a plain sum overshoots when the points are close together.)
 * The manifold's entry for a body is (dv, dw) = (v_copy - v, w_copy - w) of that body's copy after the last pass; a manifold
 * in which no visit applied an impulse makes no entry.
 * Jacobi over the manifolds, as the position pass over its points: every body reads the post-derive state of all bodies, adds
 * the entries of its touching neighbours in neighbour index order, each sum starting from 0, and then v += dv / count,
 * w += dw / count (count = number of entries as a double; nothing happens when it is 0).  Both bodies of a pair compute the
 * same sequence on the same values, so they apply opposite impulses of the same size.
 * Ground, after the body's pair entries have been applied, sequentially per body as collision::ground: for every set bit of
 * the substep's ground contact mask in ascending vertex order, p = frame * vertex with frame the body's Rigid::frame() at
 * (x, q), n = (0, 0, 1), vn = dot(n, u(p)), vn0 = dot(n, u0(p)) with the body's CURRENT v, w (v0, w0 never change),
 * Wsum = W(p, n); the vertex makes an entry iff  e > 0 && vn0 < -bounce_threshold && Wsum > 0 && vn < (-e) * vn0, with
 * lambda = ((-e) * vn0 - vn) / Wsum and P = lambda * n applied at once, so that the next vertex sees the updated velocities
 * (one pass, no give-back).
 * The impulse of a contact point is never attractive.  A contact with e == 0 makes no entry and does not count, so a world without
 * restitution, or with every coefficient 0, steps bit for bit as before (it runs the same kernels in the same order), and so
 * does every joint, limit, filter, report, ray cast and history call.  Positions and rotations are not touched by the pass.
 * Defaults: restitution == NULL with n == 0 sets every body to 0 (ground_restitution and bounce_threshold still apply);
 * otherwise n must equal xpbd_world_body_count, the caller's order.
 * Lifetime: xpbd_world_upload_bodies resets every coefficient and the threshold to 0; xpbd_world_set_joints,
 * xpbd_world_set_materials, history push / restore and mode changes leave them alone.  XPBD_MODE_FUSED / _PER_SUBSTEP accept
 * the call and ignore the values.
 * XPBD_E_INVALID (the previous values stay in place): a NULL world, restitution == NULL with n > 0, restitution != NULL with
 * n not equal to the body count, a coefficient outside [0, 1] or NaN (ground_restitution included), a negative, infinite or
 * NaN bounce_threshold.
 * Not here: xpbd_multi_world_* has no such call (a shard steps its ghosts without the ghosts' own neighbours, so a ghost's
 * post-derive velocity is not its owner's: the pass needs a second exchange per substep); joints and joint limits do not
 * bounce; xpbd_material is unchanged. */
#define XPBD_RESTITUTION_SWEEPS 4u   /* passes over the points of one manifold */
int  xpbd_world_set_restitution(xpbd_world *w, const double *restitution, uint32_t n, double ground_restitution,
                                double bounce_threshold);

/* DAMPING (EXTENSION): body drag, speed caps and joint dampers, a velocity pass after derive.
 * Every body has a row {linear c_l, angular c_a, max_linear_speed, max_angular_speed}: drag coefficients >= 0 (1/s, finite,
 * default 0) and caps > 0 (m/s, rad/s; +inf allowed and the default: no cap).  A joint of the last xpbd_world_set_joints may
 * have a damper {linear mu_l, angular mu_a}, both >= 0 (1/s, finite; a joint that is not listed has 0, 0): with a compliant
 * ANGLE / POSITION drive as the spring this is the D-term of a PD controller (Mueller et al. 2020, 3.5).
 * Where: XPBD_MODE_CONTACTS only, as stage 7 of every substep, after stage 6 (RESTITUTION) or, with restitution off, after
 * Rigid::derive, under both narrowphases; xpbd_world_step and xpbd_world_contacts_substep run it alike.  It changes the two
 * velocities of every body that is awake (SLEEPING) and not FIXED (inverse_mass and all nine inverse_inertia entries == 0, the
 * islands' definition) and nothing else: a fixed body -- a kinematic one included -- keeps its velocities to the bit, a
 * sleeper stays frozen, and no position or rotation is touched.
 * Notation.  h: the substep; x, q, v, w: a body's position, rotation, velocity and angular velocity as stage 6 left them;
 * c = x + center_of_mass.  u(p), W(p, n), dot, length and "an impulse P at p" are those of RESTITUTION, at these values:
 *   u(p) = v + cross(w, p - c)      W(p, n) = inverse_mass + dot(inverse_inertia * a, a),  a = conjugate(q) * cross(p - c, n)
 *   P at p changes the body's velocities by   dv = P * inverse_mass,   dw = cross(inverse_inertia * (p - c), P)
 * Every / is a correctly rounded division and every length a correctly rounded sqrt, nothing is contracted, and a reciprocal
 * is formed first and then multiplied where the text writes x * (1.0 / y).
 * 1. Joint dampers, Jacobi over the joints in the convention of the position pass: every body reads x, q, v, w of ALL bodies
 *    as stage 6 left them (nobody sees a neighbour's stage-7 result) and walks its joints in ascending joint index.  For joint
 *    j with mu_l, mu_a not both 0 and ends a, b: p_a, p_b are the world anchors as the joint pass forms them (Rigid::frame() of
 *    the end at x, q, times the anchor), and for each of the two coefficients  k = (mu * h < 1.0) ? mu * h : 1.0.
 *      linear (mu_l > 0):   d = u_b(p_b) - u_a(p_a), len = length(d); no term if len == 0.  n = d * (1.0 / len),
 *        Wsum = W_a(p_a, n) + W_b(p_b, n); no term unless Wsum > 0.  lambda = (k_l * len) / Wsum.  The term changes a by the
 *        impulse P = lambda * n at p_a and b by the impulse (-lambda) * n at p_b (dv and dw as above).
 *      angular (mu_a > 0), on the SAME stage-6 velocities (not on the linear term's result):  d = w_b - w_a, len = length(d);
 *        no term if len == 0.  n = d * (1.0 / len), Wang = dot(inverse_inertia_a * n_a, n_a) + dot(inverse_inertia_b * n_b, n_b)
 *        with n_a = conjugate(q_a) * n, n_b = conjugate(q_b) * n (the angular w of the limits); no term unless Wang > 0.
 *        lambda = (k_a * len) / Wang.  The term changes a by  dw = q_a * (inverse_inertia_a * (conjugate(q_a) * (lambda * n)))
 *        and b by  dw = q_b * (inverse_inertia_b * (conjugate(q_b) * ((-lambda) * n))).
 *    The joint's ENTRY for a body is (dv, dw), each the sum, started from 0, of the changes its terms make to that body, the
 *    linear term's first; a joint with no term makes no entry.  A body adds the entries of its joints, each sum started from 0,
 *    and with count = the number of entries as a double, nonzero:  v = v + dv / count,  w = w + dw / count.
 *    Both ends of a joint evaluate the same expressions on the same values, so a term's two impulses are opposite and of one
 *    size; the division by count is per body, so where the two ends' counts differ the impulses they APPLY differ, as in the
 *    position pass (the damper then removes less relative velocity than k asks for, never more).
 * 2. Drag, implicit and unconditionally stable:  s_l = 1.0 / (1.0 + h * c_l),  v = v * s_l  per component; likewise w with
 *    s_a = 1.0 / (1.0 + h * c_a).  c == 0 gives s == 1.0, which leaves every bit.  After S substeps a free body's velocity is
 *    v0 multiplied S times by s; while (S + 1) h c <= 4 / 3 it exceeds v0 * exp(-c S h) by at most S (h c)^2 / 2, relative
 *    (tests/test_damping_model.py derives it).
 * 3. Caps:  m = length(v);  if (m > max_linear_speed) v = v * (max_linear_speed / m);  likewise w with max_angular_speed.
 *    +inf never fires; afterwards length(v) <= cap up to the two roundings per component.
 * Off means off: the pass is on -- and the step then runs the unfused schedule, as with restitution -- only while some body
 * row differs from the default or the joint list holds a nonzero coefficient.  Otherwise the step launches exactly what it
 * launched before; a call of either setter with all defaults turns the pass off again.
 * xpbd_world_set_damping: rows == NULL with n == 0 gives every body the default row; otherwise n must equal
 * xpbd_world_body_count, the caller's order.  xpbd_world_get_damping returns the rows in force (n = the body count).
 * xpbd_world_set_joint_damping replaces the whole list (n == 0 clears it); at most one entry per joint.
 * Lifetime.  The rows are a body-indexed setting like materials and restitution: xpbd_world_upload_bodies resets them,
 * xpbd_world_remove_bodies(_device) keeps the survivors' rows, xpbd_world_add_bodies gives the new bodies the default row; mass
 * edits, history push / restore and the joint setters leave them alone.  The joint list names joints by index like limits and
 * drives: xpbd_world_set_joints and xpbd_world_upload_bodies clear it, xpbd_world_set_joint_limits, _set_joint_drives and
 * _set_drive_targets leave it alone, a population change re-indexes it with the joints.  With sleeping on both setters wake
 * every body.  XPBD_MODE_FUSED / _PER_SUBSTEP accept xpbd_world_set_damping and ignore the values.
 * XPBD_E_INVALID (the previous values stay in force): a NULL world; NULL rows / list with n > 0; n not equal to the body count
 * (set_damping with rows, get_damping); a negative, NaN or infinite coefficient; a cap that is <= 0 or NaN;
 * xpbd_world_set_joint_damping with n > 0 on a world not in XPBD_MODE_CONTACTS; a joint index out of range; two entries for
 * one joint; reserved != 0.  After a failed call (XPBD_E_OOM, XPBD_E_HIP) the previous values are still in force.
 * Not here: the multi-GPU world (a ghost's post-derive velocity is not its owner's: restitution's reason); editing rows in
 * place or on the device; the pinned reference modes; drives on ball joints; joint reactions; sleeping of part of a group. */
typedef struct xpbd_body_damping {   /* 32 bytes */
    double linear;             /* c_l >= 0, 1/s, default 0 */
    double angular;            /* c_a >= 0, 1/s, default 0 */
    double max_linear_speed;   /* > 0, +inf allowed = default: no cap (m/s) */
    double max_angular_speed;  /* > 0, +inf allowed = default: no cap (rad/s) */
} xpbd_body_damping;
int  xpbd_world_set_damping(xpbd_world *w, const xpbd_body_damping *rows, uint32_t n);   /* NULL, 0: all defaults */
int  xpbd_world_get_damping(xpbd_world *w, xpbd_body_damping *rows, uint32_t n);
typedef struct xpbd_joint_damping {  /* 24 bytes */
    uint32_t joint, reserved;  /* index into the list of the last xpbd_world_set_joints; reserved must be 0 */
    double   linear;           /* mu_l >= 0, 1/s */
    double   angular;          /* mu_a >= 0, 1/s */
} xpbd_joint_damping;
int  xpbd_world_set_joint_damping(xpbd_world *w, const xpbd_joint_damping *list, uint32_t n);   /* whole list; n == 0 clears */

/* TERRAIN (EXTENSION): a heightfield as the ground of the contact pipeline, in place of the reference's plane z = 0.
 * A grid of nx * ny heights over the world's x, y plane; every cell is split along its (0,0)-(1,1) diagonal into two triangles,
 * and the ground under a point is the PLANE of the triangle above or below it.  Ground contacts stay vertex against plane, at
 * most one per shape vertex, so the contact mask, xpbd_world_download_contacts, XPBD_FLAG_TRACE_CONTACTS, the history and the
 * frame snapshot keep their shape; only the plane under each vertex changes.
 * Lookup, the one definition every user of the terrain shares (dot, length and reciprocal-then-multiply as everywhere else,
 * correctly rounded / and sqrt, nothing contracted).  For a world point x, with x0, y0 = origin and dx, dy = cell:
 *   1. u = (x.x - x0) / dx, v = (x.y - y0) / dy.  Unless u >= 0 && v >= 0 the point is OUTSIDE (so a NaN is outside).
 *   2. fi = floor(u), fj = floor(v), as doubles.  Unless fi < nx - 1 && fj < ny - 1 the point is outside: the field is
 *      half-open at its far edges.  Only then i = fi, j = fj as integers.
 *   3. fu = u - fi, fv = v - fj; h00 = H[j][i], h10 = H[j][i+1], h01 = H[j+1][i], h11 = H[j+1][i+1]  (H[j][i] = heights[j * nx + i]).
 *   4. fu >= fv, the lower triangle h00, h10, h11:  sx = (h10 - h00) / dx, sy = (h11 - h10) / dy;
 *      otherwise the upper triangle h00, h11, h01:  sx = (h11 - h01) / dx, sy = (h01 - h00) / dy.
 *   5. raw = (-sx, -sy, 1.0), n = raw * (1.0 / length(raw)).
 *   6. d = dot(n, (x0 + fi * dx, y0 + fj * dy, h00)).  The plane is {n, d}; s = dot(n, x) - d is the signed distance of x
 *      (src/geometry.rs:39-41).
 * (The device keeps n and d of both triangles of every cell, evaluated once by the setter with exactly these operations: 64
 * bytes per cell, at most 256 MiB.  The heights are kept beside it for the terrain distance queries, which measure against the
 * samples themselves: 8 bytes per sample, at most 32 MiB.)
 * Ground contacts (XPBD_MODE_CONTACTS only), collision::ground with a terrain: vertex v with x = frame * vertex contacts iff
 * x is inside the field and !(s >= 0.0); its target = x - s * n per component, where the reference has {x.x, x.y, 0.0}.
 * Everything after `target` is unchanged, operation by operation: correction, delta, delta_tangential, the friction factor,
 * c1, the depenetration limit, W, lagrange, the impulse.  A vertex outside the field has NO ground contact: the terrain
 * replaces the plane, and beyond it there is nothing.  A field with every height 0 therefore steps bodies that stay over it
 * bit for bit as the plane does.
 * Vertex against plane misses a terrain ridge that pokes into a body's FACE between its vertices; the reference's ground
 * misses nothing only because a plane is flat.  Choose cells no smaller than the bodies that are to lie on them.
 * Restitution's ground part with a terrain: for every set bit of the mask in vertex order p is formed as before, the lookup
 * is repeated at p (outside the field: the vertex makes no entry) and n is the plane's normal in place of (0, 0, 1); the rest
 * is unchanged.
 * xpbd_world_sample_terrain takes HOST arrays and waits; it is evaluated on the device from the table the stepper reads.
 * For point k = (x, y) = xy[2k], xy[2k+1], the lookup at (x, y, 0): inside the field height[k] = (d - (n.x * x + n.y * y)) / n.z
 * and normal_xyz[3k..3k+2] = n; outside (NaN included) height[k] = NaN and the normal is (0, 0, 0).  normal_xyz may be NULL.
 * Hosts place bodies on the ground with it.  XPBD_E_INVALID without a terrain, or with NULL xy / height and n > 0.
 * Lifetime: world-level, as the contact pad: the terrain survives xpbd_world_upload_bodies, population changes, history
 * restore, the joint and material setters and mode changes.  XPBD_MODE_FUSED and XPBD_MODE_PER_SUBSTEP (the pinned reference
 * path) accept the call and ignore the terrain, as they ignore materials.  hf == NULL: back to the plane z = 0.  The heights
 * are copied.  The call waits for queued substeps.  With a terrain xpbd_world_step runs the substeps one kernel sequence each
 * (as with restitution on) instead of fusing the end of one with the start of the next; a world without one runs the same
 * kernels in the same order as before.
 * XPBD_E_INVALID, the previous terrain staying in force: a NULL world, nx or ny below 2, more than XPBD_MAX_TERRAIN_SAMPLES
 * samples, NULL heights, a non-finite height, origin or cell, a cell <= 0.  After XPBD_E_OOM / XPBD_E_HIP the previous
 * terrain still holds too: the new table is built in a block of its own and moved in last.
 * Not here: xpbd_multi_world_* has no such call (its frame runs the fused pair-solve + integrate + ground kernel at the halo
 * seam, which has no terrain form); the contact report lists body pairs only.  Rays, overlaps and sweeps see the terrain
 * when asked to: "Terrain in the scene queries", XPBD_QUERY_TERRAIN; distance queries through xpbd_world_terrain_distance. */
#define XPBD_MAX_TERRAIN_SAMPLES (1u << 22)
typedef struct xpbd_heightfield {   /* 48 bytes */
    uint32_t nx, ny;          /* samples along x and y, each >= 2, nx * ny <= XPBD_MAX_TERRAIN_SAMPLES */
    double   origin[2];       /* world x, y of sample (0, 0) */
    double   cell[2];         /* spacing along x and y: finite, > 0 */
    const double *heights;    /* ny rows of nx: heights[iy * nx + ix], all finite; copied */
} xpbd_heightfield;
int  xpbd_world_set_terrain(xpbd_world *w, const xpbd_heightfield *hf);   /* NULL: back to the plane z = 0 */
int  xpbd_world_sample_terrain(xpbd_world *w, const double *xy, uint32_t n, double *height, double *normal_xyz);

/* Split form of xpbd_world_step(w, dt, n) in XPBD_MODE_CONTACTS, for hosts that exchange halo
 * bodies between substeps (multi-GPU):  begin(dt); n x { substep(dt / n); <exchange> }.
 * begin runs the broadphase for the coming frame; substep is one substep of the pipeline. */
int  xpbd_world_contacts_begin(xpbd_world *w, double dt);
int  xpbd_world_contacts_substep(xpbd_world *w, double h);
/* Halo exchange helpers.  dev_indices: DEVICE pointer to n body indices; dev_buf: DEVICE pointer
 * to n x 13 doubles, body-major, in the SoA field order position[3] rotation{s,x,y,z}
 * velocity[3] angular_velocity[3].  Both run asynchronously on the world's stream, so a
 * collective enqueued on the same stream (or ordered after it) sees the data. */
int  xpbd_world_export_dynamic(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, double *dev_buf);
int  xpbd_world_import_dynamic(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_buf);
/* As import_dynamic, but body dev_indices[k] takes row dev_rows[k] of dev_buf: the output of an all-gather (every
 * rank's boundary bodies back to back) is imported as it is, without a gather pass of the host framework. */
int  xpbd_world_import_dynamic_rows(xpbd_world *w, const uint32_t *dev_indices, const uint32_t *dev_rows, uint32_t n,
                                    const double *dev_buf);

/* Halo validity for hosts that run their own exchange loop: dev_snapshot[3k..3k+2] = position of body dev_indices[k] (at
 * plan time), and later *dev_max = max(*dev_max, max_k scale_k * |position_k - snapshot_k|^2) -- the largest squared distance
 * any listed body has travelled (a NaN position counts as +inf); dev_scale is optional (NULL: 1), e.g. 1 / allowance_k^2,
 * which makes the result the largest fraction of its allowance any body has used.  Device pointers; asynchronous on the
 * world's stream. */
int  xpbd_world_snapshot_positions(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, double *dev_snapshot);
int  xpbd_world_max_displacement2(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_snapshot,
                                  const double *dev_scale, double *dev_max);

/* ---------------------------------------------------------------------------
 * Multi-GPU world (EXTENSION): the caller is still World::integrate (src/world.rs:34-43), now over an N-body
 * world in XPBD_MODE_CONTACTS whose bodies are sharded over the GPUs of one node.  The caller numbers its bodies as it likes:
 * OWNERSHIP IS THE LIBRARY'S.  The bodies are binned into a uniform grid (cell edge = 2 * (largest bounding radius +
 * contact_pad + halo_margin)), the cells are ordered by spatial-hash cell key, longest axis of the world first, and that
 * sequence is cut into n_ranks runs of near-equal body count: every rank owns a slab of space across the world's longest
 * axis.  A re-plan moves the bodies that crossed a cut to their new owner and cuts the slabs anew once a shard is a tenth of
 * a share out of balance; the bodies stay on the devices through every plan.  Bodies keep the caller's numbering everywhere
 * in this interface.
 * One xpbd_multi_world drives this process's LOCAL shards of the n_ranks shards of the world: all of them (one process owns
 * every GPU) or one each (one process per GPU).  Every shard steps its owned bodies plus ghost copies of the remote
 * bodies within reach, and after EVERY substep the boundary bodies' 13 dynamic doubles travel in ONE all-gather (RCCL over
 * xGMI; XPBD_TRANSPORT_LOCAL = peer copies inside one process, also the single-GPU rehearsal with several shards on one
 * device).  The library builds the halo plan itself (no rank holds the global scene) and checks at the END of every frame,
 * over all ranks, how much of its travel allowance any body has used since the plan (halo_margin next to a shard boundary,
 * halo_margin + half a cell edge for a body more than two cells away from every foreign one).  Beyond it a remote contact
 * may have been missed in that frame, so the frame is UNDONE (the state it started from is kept aside on the device) and
 * either run again after a re-plan (XPBD_MULTI_AUTO_REPLAN, which also re-plans pre-emptively when another frame like the
 * last one would outrun the allowance) or reported as XPBD_E_HALO with the frame's start state in place.  Result: bit-identical to one xpbd_world over the same bodies
 * in the same order -- a state with possibly missed contacts never reaches the caller.
 *
 * Collective calls (create, upload, step, replan, download) must be made by every rank in the same order.  Failure model: a
 * rank that fails LOCALLY inside upload / replan / step / download (out of memory, a launch error) still takes part in the
 * call's collectives, each of which carries every rank's status, so EVERY rank returns an error from that call (the failing
 * rank its own, the others the same code with a message naming the rank) and a failed frame is undone everywhere.  A plan
 * (upload, replan, the re-plans of a step) that fails before any shard has been re-packed leaves the previous plan and the
 * state in place; one that fails while the shards are being re-packed leaves nothing to go back to: every later call on that
 * world fails then, destroy it.  If a collective itself cannot be enqueued the communicator is aborted (ncclCommAbort: blocked peers return with an error) and
 * every later call on that world fails: destroy it.  So does a host allocation failure inside any xpbd_multi_world_* call.  Argument errors are returned before any collective: the ranks' hosts
 * pass consistent arguments.  A rank that never reaches xpbd_multi_world_create leaves its peers waiting inside RCCL's
 * bootstrap; only the host's launcher can detect that.
 * Threading: xpbd_multi_world_step waits once for the broadphase's pair counts (all shards' broadphases are enqueued before
 * the first wait) and, with n_ranks > 1, for the end of the frame (the validity check).  A world with several LOCAL shards
 * enqueues their frames from one host thread per shard (started by the first step, joined by destroy): a frame is ~20 runtime
 * calls per shard and substep, more than one thread can issue for 8 GPUs in the time the GPUs need to run them.  The caller
 * still uses the world from one thread at a time.
 * The RCCL transport has run on hardware with a ONE-rank communicator only (the build box has one GPU and RCCL refuses two
 * ranks on one device); everything else is verified with XPBD_TRANSPORT_LOCAL.
 * ------------------------------------------------------------------------- */
#define XPBD_COMM_ID_BYTES 128u         /* sizeof(ncclUniqueId) */
#define XPBD_TRANSPORT_RCCL  0u
#define XPBD_TRANSPORT_LOCAL 1u         /* needs n_local == n_ranks */
#define XPBD_MULTI_AUTO_REPLAN 1u
#define XPBD_MULTI_PLAN_THROUGH_DEVICE 2u /* diagnostics: the plan-time all-gathers go through the device transport even when
                                           * every rank lives in this process (the path a one-process-per-GPU run takes) */
#define XPBD_MULTI_FULL_PLANS 8u          /* diagnostics: every re-plan re-cuts the shards from the cell keys of the WHOLE world
                                           * (default: only the first plan and a re-plan that finds the shards a tenth of a share
                                           * out of balance do; the others keep the cuts and exchange the rims of the shards only) */

typedef struct xpbd_multi_config {
    uint32_t struct_size;   /* = sizeof(xpbd_multi_config) */
    uint32_t n_ranks;       /* shards of the whole world (<= 64) */
    uint32_t first_rank;    /* global rank of this process's first shard */
    uint32_t n_local;       /* shards driven by this process: ranks [first_rank, first_rank + n_local) */
    const int32_t *devices; /* n_local HIP device ordinals */
    uint32_t transport;     /* XPBD_TRANSPORT_* */
    uint32_t flags;         /* XPBD_MULTI_* */
    const uint8_t *comm_id; /* RCCL: XPBD_COMM_ID_BYTES from xpbd_comm_unique_id, the same on every rank */
    double   contact_pad;   /* as xpbd_world_set_contact_pad (default 0.02) */
    double   halo_margin;   /* how far a body may travel between plans (default 0.5 m) */
    uint32_t narrowphase;   /* XPBD_NARROWPHASE_* */
    uint32_t reserved;      /* must be 0 */
} xpbd_multi_config;

typedef struct xpbd_multi_world xpbd_multi_world;

/* One rank creates the communicator id; the host hands it to every rank (any channel) before xpbd_multi_world_create. */
int  xpbd_comm_unique_id(uint8_t id[XPBD_COMM_ID_BYTES]);
/* The RCCL library the collectives are bound to at run time (a copy already loaded into the process is preferred over
 * loading a second one), or NULL if none could be loaded. */
const char *xpbd_comm_library(void) XPBD_NOEXCEPT;
void xpbd_multi_config_default(xpbd_multi_config *cfg) XPBD_NOEXCEPT;
int  xpbd_multi_world_create(xpbd_multi_world **out, const xpbd_multi_config *cfg);   /* collective over all ranks (RCCL) */
void xpbd_multi_world_destroy(xpbd_multi_world *mw) XPBD_NOEXCEPT;
int  xpbd_multi_world_set_polytopes(xpbd_multi_world *mw, const xpbd_polytope *shapes, uint32_t n_shapes);
int  xpbd_multi_world_set_max_depenetration_speed(xpbd_multi_world *mw, double speed);   /* as xpbd_world_set_max_depenetration_speed */
/* bodies: the slice of the caller's bodies this process HANDS OVER = global indices [first_global, first_global + n_bodies) of
 * n_global (rank r hands over the r-th of n_ranks near-equal contiguous ranges, the first n_global % n_ranks one body longer;
 * any order -- which rank ends up owning a body is decided by where the body is); joints: ALL joints of the world with GLOBAL
 * body indices, the same list on every rank.  A non-finite position is XPBD_E_INVALID (the body cannot be placed in the
 * grid).  Collective: cuts the shards, moves every body to its owner and builds the halo plan. */
int  xpbd_multi_world_upload(xpbd_multi_world *mw, const xpbd_rigid *bodies, const uint32_t *shape_id, uint32_t first_global,
                             uint32_t n_bodies, uint32_t n_global, const xpbd_joint *joints, uint32_t n_joints);
/* xpbd_world_set_joint_limits for the joints of the last upload (GLOBAL joint indices, the same list on every rank); upload
 * clears them.  Checked against those joints before any device work; not collective.  A device failure while the limits are
 * handed to the local shards leaves the shards disagreeing: the world is unusable then (destroy it). */
int  xpbd_multi_world_set_joint_limits(xpbd_multi_world *mw, const xpbd_joint_limit *limits, uint32_t n_limits);
/* xpbd_world_set_joint_drives for the joints of the last upload (GLOBAL joint indices, the same list on every rank); upload
 * clears them.  Checked against those joints before any device work; not collective.  Lifetime and errors as
 * xpbd_multi_world_set_joint_limits. */
int  xpbd_multi_world_set_joint_drives(xpbd_multi_world *mw, const xpbd_joint_drive *drives, uint32_t n_drives);
/* xpbd_world_set_collision_filters for the whole world: n_global filters in GLOBAL body order, the same list on every rank;
 * upload clears them.  Every shard gets the filters of the bodies it owns and mirrors.  Not collective. */
int  xpbd_multi_world_set_collision_filters(xpbd_multi_world *mw, const xpbd_collision_filter *filters, uint32_t n_global,
                                            uint32_t flags);
/* xpbd_world_set_materials for the whole world: n_global materials in GLOBAL body order, the same list on every rank; upload
 * resets them.  Every shard gets the coefficients of the bodies it owns and mirrors (a ghost's coefficient enters the min),
 * and they follow the bodies through re-plans and migration.  Not collective. */
int  xpbd_multi_world_set_materials(xpbd_multi_world *mw, const xpbd_material *materials, uint32_t n_global, double ground_friction);
/* xpbd_world_step(dt, substeps) of the whole sharded world; collective.  XPBD_E_HALO: see above (the frame was undone). */
int  xpbd_multi_world_step(xpbd_multi_world *mw, double dt, uint32_t substeps);
/* Re-cuts the shards from the bodies' current positions (re-balancing them), migrates bodies whose owner changed and
 * re-plans the halos.  Collective; clears XPBD_E_HALO. */
int  xpbd_multi_world_replan(xpbd_multi_world *mw);
int  xpbd_multi_world_synchronize(xpbd_multi_world *mw);
/* The slice this process handed over, [first_global, first_global + n), in the caller's order.  Collective (with more than
 * one process every owner's bodies travel in one all-gather: use download_owned on large worlds). */
int  xpbd_multi_world_download(xpbd_multi_world *mw, xpbd_rigid *out, uint32_t n);
/* The bodies this process's shards OWN at the moment, with their global indices (ids[k] belongs to out[k]); *n_out receives
 * their number even when it exceeds cap (then XPBD_E_CAPACITY).  Not collective. */
int  xpbd_multi_world_download_owned(xpbd_multi_world *mw, uint32_t *ids, xpbd_rigid *out, uint32_t cap, uint32_t *n_out);
/* out = {bodies of the world, owned here, ghosts here, boundary bodies here, rows per rank of the all-gather, plans made};
 * *max_displacement (optional) = the largest fraction of its travel allowance any body had used at the last check, in
 * margin-equivalent metres (x halo_margin). */
int  xpbd_multi_world_halo_stats(xpbd_multi_world *mw, uint64_t out[6], double *max_displacement);
/* out = {plans made, frames undone (halo violations), bodies that changed owner at the last plan, fewest / most bodies owned
 * by a rank, step calls, and the host time inside them in ns: enqueueing, waiting for the broadphases' pair counts, waiting
 * for the end of the frame; the host time of all plans (creation and re-plans) in ns; how many of the plans were full ones
 * (shards re-cut from the cell keys of the whole world) and how many light ones (cuts kept, only the rims exchanged)}. */
int  xpbd_multi_world_plan_stats(xpbd_multi_world *mw, uint64_t out[12]);
/* owner[g] = rank that owns body g as of the last plan (n_global entries).  COLLECTIVE when ranks live in other processes. */
int  xpbd_multi_world_owners(xpbd_multi_world *mw, uint8_t *owner, uint32_t n_global);
int  xpbd_multi_world_contact_stats(xpbd_multi_world *mw, uint64_t out[3]);             /* sums of xpbd_world_contact_stats */
/* Diagnostics, host only (no device needed), exactly as the plans compute them.  The grid cell key of a bounding-sphere
 * centre; the owner of every body from the cell keys of all bodies (the keys
 * re-packed with the longest axis of the cells' bounding box first, that sequence cut into n_ranks runs of near-equal body count, on cell boundaries unless a rank would end up more than a quarter
 * of its share off balance -- then the cell is split by body index); and one rank's halo plan from keys and owners (ascending
 * ghost ids: the remote bodies it mirrors; ascending boundary ids: its own bodies that others mirror; far (optional): per
 * owned body in ascending index, 1 if no foreign body lies within two cells, so that it may travel halo_margin + half a cell
 * edge before the halos must be re-planned, the others halo_margin). */
int64_t xpbd_halo_cell_key(const double centre[3], double cell_edge) XPBD_NOEXCEPT;
int  xpbd_halo_partition(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint8_t *owner);
int  xpbd_halo_plan_owned(const int64_t *cell_keys, const uint8_t *owner, uint32_t n_global, uint32_t n_ranks, uint32_t rank,
                          const xpbd_joint *joints, uint32_t n_joints, uint32_t *ghosts, uint32_t *n_ghosts, uint32_t *boundary,
                          uint32_t *n_boundary, uint8_t *far, uint32_t cap);
/* One rank's LIGHT plan, as the re-plans of xpbd_multi_world compute it: the cuts are those of xpbd_halo_partition for
 * `keys_at_cut` (where the bodies were when the slabs were cut last; every body is still held by the rank that owned it then),
 * a body's owner now (owner_now[g], all n_global of them) follows from its present cell key and those cuts, and the rank plans
 * from the bodies it holds plus the RIMS every holder would publish (bodies within two layers of a cut, bodies that change
 * owner, ends of joints that leave their holder).  own: what the rank will own (ascending); ghosts / boundary / far as
 * xpbd_halo_plan_owned, which must give the same lists for (cell_keys, owner_now). */
int  xpbd_halo_plan_light(const int64_t *keys_at_cut, const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank,
                          const xpbd_joint *joints, uint32_t n_joints, uint8_t *owner_now, uint32_t *own, uint32_t *n_own,
                          uint32_t *ghosts, uint32_t *n_ghosts, uint32_t *boundary, uint32_t *n_boundary, uint8_t *far, uint32_t cap);
/* ... the same with ownership by contiguous index ranges (rank r owns the r-th of n_ranks near-equal ranges). */
int  xpbd_halo_plan_far(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank, uint8_t *far, uint32_t cap,
                        uint32_t *n_owned);
int  xpbd_halo_plan(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank, const xpbd_joint *joints,
                    uint32_t n_joints, uint32_t *ghosts, uint32_t *n_ghosts, uint32_t *boundary, uint32_t *n_boundary, uint32_t cap);

/* State history: the device-side counterpart of the reference app's `states: Vec<(World,
 * DebugLines)>` with its `current_state` cursor (src/app.rs:48, 206-212), which lets the user
 * scrub back through every simulated frame.  `World` is `Copy` there; here a state is the 13
 * dynamic doubles per body plus the contact masks of the last substep, copied device-to-device
 * (27 MB per state at 262 144 bodies -- thousands of frames fit in HBM).
 *   push     appends the current state, *index_out (optional) = its index (= length before the call)
 *   restore  makes state `index` the current one (neighbour lists of XPBD_MODE_CONTACTS are rebuilt
 *            by the next step / contacts_begin); stepping on from it reproduces the original run
 *            bit for bit
 *   truncate drops the states with index >= length (branching off a past state)
 * xpbd_world_upload_bodies clears the history. */
int  xpbd_world_history_push(xpbd_world *w, uint32_t *index_out);
int  xpbd_world_history_restore(xpbd_world *w, uint32_t index);
int  xpbd_world_history_truncate(xpbd_world *w, uint32_t length);
uint32_t xpbd_world_history_length(const xpbd_world *w) XPBD_NOEXCEPT;

/* ---------------------------------------------------------------------------
 * Body EDITS (EXTENSION): forces, impulses and state of RESIDENT bodies, without uploading them again.  NOT in the reference,
 * whose app owns its two `Rigid`s and writes their fields directly (src/world.rs, src/app.rs); behind this ABI the bodies live
 * on the device, and xpbd_world_upload_bodies drops every body-indexed setting with them.
 *
 * What an edit acts on.  The state xpbd_world_download_bodies would return after the work already enqueued, in every mode (in
 * XPBD_MODE_CONTACTS the current state, as the ray casts see it).  An edit is ordered on the world's stream: the next
 * xpbd_world_step (or xpbd_world_contacts_begin / _substep) sees it.  An edit changes NOTHING else: joints, limits, filters,
 * materials, restitution, the contact report and its S_prev, the history entries, contact masks and neighbour lists all stay
 * (the next xpbd_world_step builds its broadphase from the edited state anyway; a host on the split API that teleports bodies
 * mid-frame calls xpbd_world_contacts_begin again).  The property everything else rests on: a world after an edit steps bit for
 * bit like a fresh world into which the edited xpbd_rigid array was uploaded (with the same settings set again).
 *
 * Index lists.  indices[k] names the body of entry k.  indices == NULL means the bodies 0..n-1, and then n must equal
 * xpbd_world_body_count.  n == 0 is XPBD_OK and does nothing.
 *
 * xpbd_world_set_external_wrench: external_force of body indices[k] = force_xyz[3k..3k+2] and external_torque =
 *   torque_xyz[3k..3k+2].  force_xyz or torque_xyz may be NULL: that field of the listed bodies is left alone (both NULL with
 *   n > 0 is XPBD_E_INVALID: nothing to set).  The values REPLACE the old ones and stay until they are replaced again: they are
 *   two of the static fields of xpbd_rigid, so xpbd_world_history_restore does NOT bring old forces back (a history entry is
 *   the 13 dynamic doubles), and every substep integrates them as it integrates uploaded ones (Rigid::integrate, src/rigid.rs:82-99).
 *
 * xpbd_world_apply_impulses: entry k changes velocity and angular_velocity of body list[k].body, exactly as the restitution
 *   pass applies an impulse (above: v += P * inverse_mass; w += cross(inverse_inertia * arm, P)).  With c = position +
 *   center_of_mass at the body's current pose, in this order:
 *     1. velocity += impulse * inverse_mass
 *     2. unless XPBD_IMPULSE_AT_CENTRE:  arm = point - c;  angular_velocity += cross(inverse_inertia * arm, impulse)
 *     3. angular_velocity += inverse_inertia * angular_impulse      (always executed, also for a zero angular_impulse; as the
 *        hinge's angular term uses inverse_inertia * turn)
 *   per component, no fused multiply-add, dot / cross / matrix product as everywhere else.  A body may appear several times:
 *   its entries are applied one after another in list order, each on the result of the one before.  Entries of different bodies
 *   are independent.  Positions and rotations are not touched.  A body with inverse_mass == 0 and a zero inverse_inertia keeps
 *   its velocities (+ 0.0).  The host variant sorts the entries by body (stable) and runs the device path.
 *
 * xpbd_world_set_dynamics / _get_dynamics: row k = the 13 dynamic doubles of body indices[k] in the order of
 *   xpbd_world_export_dynamic: position[3], rotation {s, x, y, z}, velocity[3], angular_velocity[3].  set writes all 13 (a
 *   teleport, a stop, a throw); the rotation is taken as given (the caller keeps it a unit quaternion).  get only reads.
 *
 * Host variants (no _device suffix) take host arrays, check EVERYTHING before any device work and wait for completion, as
 * xpbd_world_raycast does.  XPBD_E_INVALID, the state exactly as it was: a NULL world; a NULL list with n > 0 (indices == NULL
 * as above excepted); a world without resident bodies; an index >= xpbd_world_body_count; the same index twice in
 * set_external_wrench / set_dynamics; unknown `flags` bits; any NaN or infinite force, torque, impulse, point (unless
 * XPBD_IMPULSE_AT_CENTRE: then `point` is ignored altogether), angular impulse or row value.
 *
 * Device variants take DEVICE arrays (e.g. a torch tensor's data_ptr()), are ordered on the world's stream
 * (xpbd_world_get_stream / _set_stream: the caller's producer runs on that stream or is ordered before it) and return before
 * completion; the arrays must stay valid until the stream has passed the call.  They cannot see the values: only NULL
 * arguments, a world without bodies, the indices == NULL form with n != body count, n > 2^29 and a dev_list that is not 16-byte
 * aligned are XPBD_E_INVALID.  An index >= body count is SKIPPED by the kernel (that entry does nothing).  Unknown flag bits are
 * ignored.  UNSPECIFIED results: the same index twice in xpbd_world_set_external_wrench_device (one of the values wins); entries
 * of one body that are not ADJACENT in xpbd_world_apply_impulses_device -- the entries of a body must form one run; every run is
 * applied by one lane, which loads the body once, walks the run in order and stores the velocities once.
 *
 * Multi world.  xpbd_multi_world_set_external_wrench / _apply_impulses take GLOBAL body indices and are checked against n_global
 * as the host variants above.  Not collective: every rank passes the same list (as xpbd_multi_world_set_materials).  Every local
 * shard applies the entries of every body it HOLDS, owned or ghost: a shard integrates its ghosts itself in the first substep
 * of a frame, so a ghost carries the force and the velocity of its owner -- the same arithmetic on the same values, the same
 * bits on every holder.  The forces are part of the body records, which travel with the bodies through re-plans and migration.
 * Before the first xpbd_multi_world_upload: XPBD_E_INVALID.  A device failure inside leaves the shards disagreeing: the world is
 * unusable then (destroy it).
 * Not here: xpbd_multi_world_set_dynamics (a teleported body interacts with the halo plan's travel allowance and needs a
 * design of its own: upload again, or move the body with impulses), device variants of the multi-world calls.  (Scripted
 * bodies that push and carry: "KINEMATIC bodies".  Changing the mass properties: "MASS properties of resident bodies".)
 * ------------------------------------------------------------------------- */
#define XPBD_IMPULSE_AT_POINT  0u   /* impulse acts at `point` (world space) */
#define XPBD_IMPULSE_AT_CENTRE 1u   /* impulse acts at position + center_of_mass; `point` is ignored */
typedef struct xpbd_impulse {       /* 80 bytes */
    uint32_t body, flags;           /* XPBD_IMPULSE_* */
    double   impulse[3];            /* N s, world space */
    double   point[3];              /* world space */
    double   angular_impulse[3];    /* N m s, world space */
} xpbd_impulse;

int  xpbd_world_set_external_wrench(xpbd_world *w, const uint32_t *indices, uint32_t n,
                                    const double *force_xyz, const double *torque_xyz);
int  xpbd_world_set_external_wrench_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n,
                                           const double *dev_force_xyz, const double *dev_torque_xyz);
int  xpbd_world_apply_impulses(xpbd_world *w, const xpbd_impulse *list, uint32_t n);
int  xpbd_world_apply_impulses_device(xpbd_world *w, const xpbd_impulse *dev_list, uint32_t n);
int  xpbd_world_set_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *rows);
int  xpbd_world_get_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, double *rows);
int  xpbd_multi_world_set_external_wrench(xpbd_multi_world *mw, const uint32_t *indices, uint32_t n,
                                          const double *force_xyz, const double *torque_xyz);   /* GLOBAL indices */
int  xpbd_multi_world_apply_impulses(xpbd_multi_world *mw, const xpbd_impulse *list, uint32_t n); /* GLOBAL bodies */

/* ---------------------------------------------------------------------------
 * MASS properties of resident bodies (EXTENSION): freeze, release, re-weigh -- the 13 mass doubles of RESIDENT bodies
 * (inverse_mass, inverse_inertia[9], center_of_mass[3]) changed in place.  NOT in the reference, whose `Rigid`s get theirs once,
 * from Rigid::new (src/rigid.rs:53-71).  The single world only.
 *
 * The property everything rests on is the one of "Body EDITS": a world after the call steps bit for bit like a fresh world into
 * which xpbd_world_download_bodies taken after the call was uploaded, with the same settings set again -- in every mode and for
 * every flag below.  Index lists, the NULL form, n == 0, the host / device split and the ordering on the world's stream are those
 * of xpbd_world_set_dynamics and xpbd_world_set_external_wrench(_device).  All arithmetic is per component, with no fused
 * multiply-add and correctly rounded divisions.
 *
 * flags = a layout (the low eight bits) | XPBD_MASS_KEEP_FRAME or not.  Row k is 13 doubles for body indices[k]:
 *   XPBD_MASS_INVERSE  inverse_mass, inverse_inertia[9] (column-major), center_of_mass[3]: the xpbd_rigid fields, taken as given;
 *                      the 13 doubles of the body become rows[13k..13k+12].
 *   XPBD_MASS_DIRECT   mass, inertia[9] (column-major, about the centre of mass), center_of_mass[3], inverted on the device as
 *                      Rigid::new does: inverse_mass = 1.0 / mass;  inverse_inertia = cgmath's Matrix3::invert of the tensor m
 *                      (columns x, y, z):  det = m.x.x * (m.y.y * m.z.z - m.z.y * m.y.z) - m.y.x * (m.x.y * m.z.z - m.z.y * m.x.z)
 *                      + m.z.x * (m.x.y * m.y.z - m.y.y * m.x.z) first, det == 0.0 is singular;  then the columns
 *                      cross(m.y, m.z) / det, cross(m.z, m.x) / det, cross(m.x, m.y) / det, transposed.  center_of_mass as given.
 *   XPBD_MASS_KEEP_FRAME (either layout): the body's geometry stays where it is when center_of_mass changes.  With com, com' the
 *                      old and the new centre of mass, d = com' - com, q the body's rotation and r = q * d (the rotation operator
 *                      of Rigid::frame):  position' = position + (r - d);  velocity' = velocity + cross(angular_velocity, r), the
 *                      velocity of the material point that becomes the centre of mass.  Rotation and angular velocity stay.
 *                      Rigid::frame() of the body is then what it was, up to the roundings of these two formulas.
 *   Without XPBD_MASS_KEEP_FRAME no dynamic double is touched: the world is what an upload of the downloaded bodies with the new
 *   13 doubles would be, and the geometry shifts if center_of_mass changed.
 * xpbd_world_get_mass_properties returns rows in the INVERSE layout, whatever layout they were set in.
 *
 * The kinematic rule.  A body with an entry in the kinematic table ("KINEMATIC bodies") stays FIXED: only a row whose inverse_mass
 * and nine inverse_inertia entries are all == 0 is taken (its center_of_mass may change).  To give it mass, clear its entry first.
 * Grab, carry, release: get the 13 doubles, set zeros (freeze), xpbd_world_set_kinematics with a target, step, clear the table,
 * set the saved doubles.  Nothing here remembers the mass from before a freeze: the caller keeps what get returned.  A frozen
 * body keeps the velocities it had, and a fixed body moves at its velocity: stop it with xpbd_world_set_dynamics if it shall stay.
 *
 * Host variants check EVERYTHING before any device work and wait for completion.  XPBD_E_INVALID, with nothing changed: a NULL
 * world; NULL rows with n > 0; no resident bodies; indices == NULL with n other than the body count; an index out of range; in
 * set, the same index twice; unknown flag bits or a layout other than 0 or 1; any non-finite row value; inverse_mass < 0; DIRECT
 * with mass <= 0; a row that breaks the kinematic rule.  DIRECT with a singular tensor is XPBD_E_SINGULAR_INERTIA, with nothing
 * changed: the code that mirrors the reference's panic.
 * The device variant takes DEVICE arrays, only enqueues and cannot see the values.  XPBD_E_INVALID: NULL arguments, no bodies,
 * dev_indices == NULL with n != body count, n > 2^29, dev_rows not 8-byte aligned, unknown flag or layout bits.  The kernel SKIPS
 * an entry -- that entry changes no body -- whose index is out of range, that has a non-finite value, a negative inverse mass or a
 * mass that is not positive, whose DIRECT determinant is == 0, or that breaks the kinematic rule.  The same index twice is
 * unspecified, but one entry wins whole: the 13 doubles (and with KEEP_FRAME the position and velocity) are never a mix of two.
 *
 * What else changes: nothing.  Joints, limits, drives, filters, materials, restitution, the kinematic table, the contact report
 * and its S_prev, contact masks and the history entries stay.  A history entry carries only dynamic doubles, so the edited mass
 * STAYS after xpbd_world_history_restore, as an external wrench does (a KEEP_FRAME shift of position and velocity is dynamic state
 * and is restored away with the rest).  A population change carries the edited doubles with the body.  xpbd_world_islands reads the
 * mass properties per call: a body made fixed is an anchor from the next call on.  A host on the split API calls
 * xpbd_world_contacts_begin again after a mass edit (xpbd_world_contacts_substep refuses until then), and
 * xpbd_world_download_neighbours waits for the next broadphase too.  The contact pipeline reads the mass properties through a
 * per-shape table while all bodies of a shape share theirs bit for bit; an edited world reads per-body records instead, same
 * values and same bits, until the next xpbd_world_upload_bodies.
 * SLEEPING: as every edit, naming a sleeper wakes its group at the start of the next step and naming a FIXED body wakes everybody
 * (an anchor changed) -- judged by the mass properties from BEFORE the edit, so releasing a frozen body wakes everybody, and
 * freezing a sleeper wakes its group: the new fixed body is inert from then on and never asleep again, and what rested on it may
 * go back to sleep anchored to it.  An entry the device variant skips may still wake its body's group (a wake is always safe).
 * Not here: the multi-GPU world; a shadow copy of the mass from before a freeze (the caller keeps the 13 doubles get returned);
 * sharing the per-shape table again after an edit; deriving mass from a shape and a density on the device (the host mirror's
 * rigid_metrics does that, and its result is a DIRECT row).
 * ------------------------------------------------------------------------- */
#define XPBD_MASS_INVERSE    0u     /* row = inverse_mass, inverse_inertia[9] (column-major), center_of_mass[3]: taken as given */
#define XPBD_MASS_DIRECT     1u     /* row = mass, inertia[9] (column-major, about the centre of mass), center_of_mass[3]: inverted on the device */
#define XPBD_MASS_KEEP_FRAME 0x100u /* the body's geometry stays where it is when center_of_mass changes */
int  xpbd_world_set_mass_properties(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *rows /* [n][13] */, uint32_t flags);
int  xpbd_world_set_mass_properties_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_rows, uint32_t flags);
int  xpbd_world_get_mass_properties(xpbd_world *w, const uint32_t *indices, uint32_t n, double *rows /* [n][13], always the INVERSE layout */);

/* ---------------------------------------------------------------------------
 * Body POPULATION (EXTENSION): removing RESIDENT bodies and appending new ones, without uploading the others again.  NOT in
 * the reference, whose world is a fixed pair of `Rigid`s (src/world.rs).  xpbd_world_upload_bodies is the other way to change
 * the population, and it drops every body-indexed setting; here everything that belongs to a surviving body survives with it,
 * re-indexed, and the work stays on the device: a scan of the removal flags, one SoA -> SoA gather of the bodies and one
 * gather per per-body table.
 *
 * Order.  The survivors keep their relative order and are packed to the front: old_to_new[i] is the number of survivors among
 * the bodies 0..i-1; a removed body maps to XPBD_NO_HIT (0xFFFFFFFF).  Added bodies are appended in the caller's order;
 * *first_index_out is the body count before the call.  There are no handles: the maps are the contract.
 *
 * What travels with a surviving body.  All 38 doubles of its xpbd_rigid (external and internal forces among them, so whatever
 * xpbd_world_set_external_wrench wrote), its shape id, and its row of the collision-filter table, the friction table and the
 * restitution table.  The world-level values stay: the XPBD_FILTER_* flags, ground_friction, ground restitution, bounce
 * threshold, contact pad, depenetration limit, narrowphase, SAT schedule, the contact report's enable flag, and the mode.
 *
 * Joints.  A joint whose two ends both survive stays, body_a and body_b re-indexed (their orientation kept).  A joint with a
 * removed end is dropped, with its limits (angular and SLIDE) and its drives.  The surviving joints keep their relative order:
 * joint_old_to_new[j] is the new number of joint j, XPBD_NO_HIT for a dropped one.  Limits and drives are re-indexed to the
 * new joint numbers and keep the caller's relative order.  The result is what xpbd_world_set_joints / _set_joint_limits /
 * _set_joint_drives would build from the re-indexed arrays.
 *
 * Added bodies get the defaults -- filter {~0u, ~0u}, friction +inf, restitution 0, no joints -- in a table that is on; a table
 * that is off stays off.  They are checked exactly as xpbd_world_upload_bodies checks its bodies (the shape id range; the
 * values of an xpbd_rigid are taken as given), take part in the per-shape test for shared mass properties as uploaded bodies
 * do, and are valid in every mode.  shape_id is required here (upload's NULL = "all shape 0" form does not exist).
 *
 * What is DROPPED, exactly as after an upload: the history (xpbd_world_history_length becomes 0) and the contact trace, the
 * contact masks of the last substep (xpbd_world_download_contacts reports none until the next step), the frame snapshot of a
 * shard, the neighbour lists and the per-pair axis caches, and the contact report's state: there are NO END events for removed
 * bodies, and the previous frame's pair list is invalid, so every pair touching in the next frame is a BEGIN.
 *
 * Calling discipline.  Every variant waits for completion and leaves a consistent world (the new body count has to reach the
 * host anyway).  xpbd_world_remove_bodies and xpbd_world_add_bodies take host arrays and check everything before any device
 * work.  xpbd_world_remove_bodies_device takes DEVICE flags, one byte per body, nonzero = remove; it is ordered on the world's
 * stream (xpbd_world_get_stream / _set_stream: the producer of dev_remove runs on that stream or is ordered before it).
 * dev_old_to_new (device, [old body count], or NULL) receives the map without a host round trip; when the world has joints the
 * map is also brought to the host for the joint re-index.  old_to_new is a host array of the OLD body count, joint_old_to_new
 * a host array of the old joint count, n_bodies_out the new body count; each may be NULL.
 *
 * The same index twice in `indices` is allowed and removes the body once.  n == 0 / n_add == 0 is XPBD_OK and changes nothing
 * at all (history and the rest stay; the maps are the identity), and so is a device call none of whose flags is set.  Removing
 * every body leaves a world of 0 bodies, as xpbd_world_upload_bodies(.., 0) does.
 *
 * XPBD_E_INVALID, with the world exactly as it was: a NULL world; a NULL list with n > 0 (dev_remove == NULL); NULL aos or
 * shape_id with n_add > 0; a world without resident bodies (remove); an index >= xpbd_world_body_count; a body count that
 * would exceed what xpbd_world_upload_bodies accepts; a bad added body, with the code xpbd_world_upload_bodies returns for it.
 * Failure.  Every new array is staged in a buffer of its own and moved over the old one only after every allocation, copy and
 * launch has succeeded: a failed call (XPBD_E_OOM, XPBD_E_HIP) leaves the previous population and settings in force.
 *
 * Not here: the multi-GPU world (global numbering across ranks and a collective re-plan need a design of their own);
 * per-call settings for added bodies (use the setters afterwards); stable handles; END events for removed bodies.
 * ------------------------------------------------------------------------- */
int  xpbd_world_remove_bodies(xpbd_world *w, const uint32_t *indices, uint32_t n,
                              uint32_t *old_to_new,        /* host [old body count] or NULL */
                              uint32_t *joint_old_to_new,  /* host [old joint count] or NULL */
                              uint32_t *n_bodies_out);     /* or NULL */
int  xpbd_world_remove_bodies_device(xpbd_world *w, const uint8_t *dev_remove, /* device [body count], nonzero = remove */
                                     uint32_t *dev_old_to_new,    /* device [old body count] or NULL */
                                     uint32_t *joint_old_to_new,  /* host, as above */
                                     uint32_t *n_bodies_out);
int  xpbd_world_add_bodies(xpbd_world *w, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n_add,
                           uint32_t *first_index_out);     /* or NULL */

/* ---------------------------------------------------------------------------
 * Scene queries (EXTENSION): the closest body along each of a batch of rays, at the bodies' current poses.  NOT in the
 * reference; its app would use it for picking under the cursor (src/app.rs, src/camera.rs).
 *
 * Poses and bodies.  A ray sees every body at the pose xpbd_world_download_bodies would return after the work already
 * enqueued, in every mode (in XPBD_MODE_CONTACTS the current state, never the other half of its double buffer).  A body is
 * the convex polytope of its shape as set by xpbd_world_set_polytopes (without polytopes: XPBD_E_INVALID; set_shapes gives
 * vertices only).  The ground plane is not a body: rays never hit it.  A body whose pose is not finite is never hit.
 *
 * One ray against one body, with f = Rigid::frame() of the body (src/rigid.rs:75-80) and inv = inverse(f) (src/frame.rs:30-37):
 *   o_l = inv * origin, d_l = inv.rotation * direction; t_lo = 0, face = XPBD_RAY_INSIDE, t_hi = max_distance;
 *   for every face k in index order, with the outward local plane P_k (Polytope::plane, src/geometry.rs:262-271):
 *     s = distance(P_k, o_l) (src/geometry.rs:39-41), v = dot(P_k.normal, d_l); if s or v is NaN the ray misses;
 *     v < 0: t_k = (-s) / v, and if t_k > t_lo then t_lo = t_k, face = k   (strict: the first maximum wins)
 *     v > 0: t_hi = min(t_hi, (-s) / v)
 *     v = 0: the ray misses if s > 0 (parallel, outside the slab)
 *   hit iff t_lo <= t_hi; point = origin + t_lo * direction (per component, no fused multiply-add), normal =
 *   f.rotation * P_face.normal.  Quotients are correctly rounded f64 divisions.
 * Per ray the smallest t wins and equal t go to the smaller body index (in xpbd_multi_world_raycast: the caller's global
 * index).  ignore_body is never hit.  A ray with a NaN or infinite component, a zero direction, or a max_distance that is
 * negative or NaN hits nothing (the call still succeeds).  A miss is {XPBD_NO_HIT, XPBD_NO_HIT, +inf, 0, 0}.
 *
 * Errors: XPBD_E_INVALID for a NULL world, NULL rays / hits with n_rays > 0, unknown flags, a nonzero `reserved` (host
 * variants: the device variant cannot see the rays).  n_rays == 0 is XPBD_OK.  A ray cast changes no body, contact list,
 * mask, history entry or plan: stepping after it gives the same bits as stepping without it.
 *
 * Method: a uniform grid of the bodies' bounding spheres built for every call (counting passes and scans), walked by every
 * ray cell by cell (3D-DDA).  Up to XPBD_RAYCAST_BRUTE_FORCE_RAYS rays take the brute-force path instead, which needs no
 * grid (picking latency).  Same bits either way.
 * ------------------------------------------------------------------------- */
#define XPBD_NO_HIT      0xFFFFFFFFu  /* xpbd_ray_hit.body when nothing was hit */
#define XPBD_RAY_INSIDE  0xFFFFFFFFu  /* xpbd_ray_hit.face when the ray starts inside (or on) the hit body */
#define XPBD_RAYCAST_BRUTE_FORCE 1u   /* diagnostics: test every ray against every body, no grid */
#define XPBD_RAYCAST_BRUTE_FORCE_RAYS 8u /* calls with at most this many rays take the brute-force path anyway */

typedef struct xpbd_ray {            /* 64 bytes */
    double   origin[3];
    double   direction[3];           /* need not be unit; distances are in units of |direction| */
    double   max_distance;           /* may be +inf */
    uint32_t ignore_body;            /* a body this ray never hits (XPBD_NO_HIT: none) */
    uint32_t reserved;               /* must be 0 */
} xpbd_ray;

typedef struct xpbd_ray_hit {        /* 64 bytes */
    uint32_t body;                   /* XPBD_NO_HIT: missed */
    uint32_t face;                   /* shape-local face index the ray enters through, or XPBD_RAY_INSIDE */
    double   distance;               /* t: point = origin + t * direction */
    double   point[3];
    double   normal[3];              /* world-space outward normal of `face`; (0,0,0) for XPBD_RAY_INSIDE */
} xpbd_ray_hit;

/* Host arrays; waits for the result. */
int  xpbd_world_raycast(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits);
/* Device arrays; stream-ordered on the world's stream, returns before completion (it waits only when its scratch has to
 * grow).  `reserved` is not checked. */
int  xpbd_world_raycast_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags,
                               xpbd_ray_hit *dev_hits);
/* Collective: every rank passes the same rays and gets all hits.  Every shard casts against the bodies it OWNS; bodies
 * and ignore_body are global indices. */
int  xpbd_multi_world_raycast(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags,
                              xpbd_ray_hit *hits);
/* The same three, against the bodies whose collision-filter group meets `mask` only ((group & mask) != 0; bodies without
 * filters are in group ~0u).  The plain calls test no group at all, so they still hit bodies of group 0. */
int  xpbd_world_raycast_masked(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, uint32_t mask,
                               xpbd_ray_hit *hits);
int  xpbd_world_raycast_masked_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags,
                                      uint32_t mask, xpbd_ray_hit *dev_hits);
int  xpbd_multi_world_raycast_masked(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags,
                                     uint32_t mask, xpbd_ray_hit *hits);

/* ---------------------------------------------------------------------------
 * Overlap queries (EXTENSION): which bodies does each of a batch of convex volumes touch, at the bodies' current poses.  NOT
 * in the reference.  A host asks before it spawns or teleports a body (is the place free?), for trigger and sensor volumes,
 * for area selection.
 *
 * Poses and frames.  The volume of query q is the convex polytope `shape` (xpbd_world_set_polytopes) at the frame {position,
 * rotation}: x_world = position + rotation * x_shape.  It takes the place of body A's Rigid::frame() in the SAT.  Body b is
 * its shape's polytope at its own Rigid::frame(), at the pose xpbd_world_download_bodies would return after the work already
 * enqueued (the state the ray casts see).  The ground plane is not a body.
 *
 * Body b is reported for query q iff, in this order:
 *   1. b is not ignore_body; with XPBD_OVERLAP_MASKED also (group_b & mask) != 0 (bodies without filters are in group ~0u;
 *      without the flag no group is tested);
 *   2. the tight bounding spheres overlap: between = frame_b * centroid_b - frame_q * centroid_q, reach = radius_q + radius_b,
 *      dot(between, between) < reach * reach (any NaN makes the comparison false: a body pose or query frame that is not
 *      finite reports nothing).  This is part of the definition, as in the contact pipeline: a pair whose spheres just miss
 *      by rounding is not reported whatever the SAT would say;
 *   3. the decision part of the SAT says "not separated": qa = face_axes_separation(volume, body), stop if qa >= 0 or NaN;
 *      qb = the same with the roles swapped, stop if qb >= 0 or NaN; qe = the best separation over the pairs of unique edge
 *      directions, stop if qe >= 0; m = max(qa, qb); the edge feature is used iff an edge pair qualified and qe > m + 1e-6,
 *      then m = qe.  feature = XPBD_FEATURE_EDGES, else XPBD_FEATURE_FACE_A if qa == m, else XPBD_FEATURE_FACE_B (A = the
 *      volume, B = the body); separation = m (< 0; penetration depth = -separation).  No contact points are computed.
 *
 * Result.  offsets[n_queries + 1] is a CSR array: the hits of query q are hits[offsets[q] .. offsets[q + 1]), in ascending
 * body index.  offsets is always complete and *n_out always receives the total number of hits (which must fit 32 bits).  If
 * the total exceeds cap the call returns XPBD_E_CAPACITY and hits holds the first cap entries of the full list.  hits == NULL
 * with cap == 0 is a pure count, and no error when the total is 0.
 *
 * Errors (host variants, before any device work; the outputs are untouched): XPBD_E_INVALID for a NULL world, NULL queries /
 * offsets / n_out with n_queries > 0, NULL hits with cap > 0, unknown flags, a nonzero `reserved`, a `shape` outside the
 * table, no polytopes set, no bodies resident.  n_queries == 0 is XPBD_OK with *n_out = 0.  An overlap query changes no body,
 * list, mask, report, history entry or plan: stepping after it gives the same bits as stepping without it.  Every mode
 * accepts it.
 *
 * Method: the per-call grid of the ray casts; per query a group of lanes walks the cells its sphere covers, counts its hits,
 * and after a scan of the counts lists them (every pair is tested twice instead of keeping a candidate list whose length
 * the host would have to learn); each query's segment is then sorted.  Same bits with XPBD_OVERLAP_BRUTE_FORCE.
 * ------------------------------------------------------------------------- */
#define XPBD_OVERLAP_BRUTE_FORCE 1u   /* diagnostics: every query against every body, no grid */
#define XPBD_OVERLAP_MASKED      2u   /* test xpbd_overlap_query.mask against the bodies' filter groups */

typedef struct xpbd_overlap_query {   /* 72 bytes */
    double   position[3];             /* frame of the volume: x_world = position + rotation * x_shape */
    double   rotation[4];             /* {s, x, y, z}, taken as given (the caller keeps it a unit quaternion) */
    uint32_t shape;                   /* index into the table of xpbd_world_set_polytopes */
    uint32_t ignore_body;             /* never reported (XPBD_NO_HIT: none) */
    uint32_t mask;                    /* with XPBD_OVERLAP_MASKED: body b answers only if (group_b & mask) != 0 */
    uint32_t reserved;                /* must be 0 */
} xpbd_overlap_query;

typedef struct xpbd_overlap_hit {     /* 16 bytes */
    uint32_t body;
    uint32_t feature;                 /* XPBD_FEATURE_*: A = the query volume, B = the body */
    double   separation;              /* < 0: the SAT's value for that feature (penetration depth = -separation) */
} xpbd_overlap_hit;

/* Host arrays; checks everything before any device work and waits for the result. */
int  xpbd_world_overlap(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags,
                        uint32_t *offsets, xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out);
/* Device arrays; stream-ordered on the world's stream, returns before completion (it waits only when its scratch has to
 * grow).  The total is dev_offsets[n_queries]; hits beyond cap are not written.  It cannot see the queries: a query with
 * `shape` outside the table reports nothing and `reserved` is not checked. */
int  xpbd_world_overlap_device(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags,
                               uint32_t *dev_offsets, xpbd_overlap_hit *dev_hits, uint32_t cap);
/* Collective: every rank passes the same queries and gets the whole answer.  Every shard answers for the bodies it OWNS;
 * body and ignore_body are global indices.  Same bits as one xpbd_world over the same bodies. */
int  xpbd_multi_world_overlap(xpbd_multi_world *mw, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags,
                              uint32_t *offsets, xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out);

/* ---------------------------------------------------------------------------
 * Sweep queries (EXTENSION): the first body each of a batch of convex volumes hits when it is moved along a segment, and
 * when, at the bodies' current poses.  NOT in the reference.  A host asks to set a body down against a pile before it spawns
 * it, for character and tool motion, for projectiles a ray is too thin for, for camera booms.
 *
 * Poses and frames.  The volume of sweep q is the convex polytope `shape` at the frame fa = {position, rotation}, translated
 * by t * direction for t in [0, max_distance]; it does not rotate.  Distances are in units of |direction|, as for rays.
 * Bodies stand still at the pose the other queries see.  The ground plane is not a body.
 *
 * One sweep against one body, with fb = Rigid::frame() of the body and d = direction.  World vertices aw = fa * a_v, bw =
 * fb * b_v; in the other's local space a_in_b = inverse(fb) * aw, b_in_a = inverse(fa) * bw; d_a = inverse(fa).rotation * d,
 * d_b = inverse(fb).rotation * d.  A list of linear constraints (s, v) -- "the separation along this axis at time t is
 * s + t * v" -- is visited in this order:
 *   1. every face k of the volume, local outward plane (n, disp), in face order:
 *        s = min_v dot(n, b_in_a_v) - disp, v = -dot(n, d_a)
 *   2. every face k of the body, in face order:
 *        s = min_v dot(n, a_in_b_v) - disp, v = dot(n, d_b)
 *   3. every pair q = i * n_dirs_b + j of unique edge directions (the first edge's v[e.1] - v[e.0] of every direction up to
 *      sign, in edge order), ascending: n = normalized(cross(fa.rotation * dir_a_i, fb.rotation * dir_b_j)), skipped unless
 *      all three components are finite; hiA, loA = max, min of dot(aw_v, n), hiB, loB the same over bw, w = dot(n, d); two
 *      constraints: first (loB - hiA, -w), then (loA - hiB, w).
 * (min and max: the first vertex's value, replaced by a later one that is smaller / larger.)  With t_lo = -inf, entering =
 * none, t_hi = max_distance, every constraint follows the ray's rule:
 *     s or v is NaN: the pair misses;
 *     v < 0: t_k = (-s) / v, and if t_k > t_lo then t_lo = t_k, entering = this constraint (strict: the first maximum wins)
 *     v > 0: t_k = (-s) / v, and if t_k < t_hi then t_hi = t_k
 *     v = 0: the pair misses if s >= 0 (a volume sliding along a body in exact touch does not hit it: the overlap query's
 *            ">= 0 is separated")
 * t = (t_lo < 0) ? 0 : t_lo, and the pair hits iff t <= t_hi.  If t_lo < 0 the volume overlaps the body at the start:
 * feature = XPBD_SWEEP_INITIAL, face = XPBD_NO_HIT, normal = (0,0,0).  Otherwise feature and normal come from `entering`; the
 * normal is in world space and points out of the body towards the volume:
 *     XPBD_FEATURE_FACE_A: face k of the volume, normal = -(fa.rotation * n_k);
 *     XPBD_FEATURE_FACE_B: face k of the body, normal = fb.rotation * n_k;
 *     XPBD_FEATURE_EDGES:  face = XPBD_NO_HIT, normal = -n if the first constraint of the pair entered, +n if the second.
 * position = sweep.position + t * direction (per component): the frame position of the volume at the impact.  Quotients are
 * correctly rounded f64 divisions, there is no fused multiply-add, dot, cross and normalized (v * (1 / sqrt(dot(v, v)))) are
 * as everywhere else.  The half-spaces are those of the Minkowski difference of the two polytopes -- the body's faces, the
 * volume's faces reversed, both signs of every edge-direction cross product; axes that are no face of it are supporting
 * planes all the same and change nothing -- so the answer is exact up to rounding, without iteration.
 *
 * Per sweep the smallest t wins and equal t go to the smaller body index (in xpbd_multi_world_sweep: the caller's global
 * index).  ignore_body is never hit; with XPBD_SWEEP_MASKED body b answers only if (group_b & mask) != 0 (bodies without
 * filters are in group ~0u; without the flag no group is tested).  A body whose pose is not finite is never hit.  A sweep
 * whose `shape` is outside the table, whose frame or direction has a NaN or infinite component, whose direction is zero or
 * whose max_distance is negative or NaN hits nothing (the call still succeeds).  A miss is {XPBD_NO_HIT, 0, XPBD_NO_HIT, 0,
 * +inf, zeros}.
 *
 * Errors (host variants, before any device work; the outputs are untouched): XPBD_E_INVALID for a NULL world, NULL sweeps /
 * hits with n_sweeps > 0, unknown flags, a nonzero `reserved`, no polytopes set, no bodies resident.  n_sweeps == 0 is
 * XPBD_OK.  A sweep changes no body, list, mask, report, history entry or plan: stepping after it gives the same bits as
 * stepping without it.  Every mode accepts it.
 *
 * Method: the per-call grid of the ray casts; a group of lanes per sweep walks the cells of the volume's centre line as a ray
 * does and, for the stretch of it inside one cell, tests the bodies listed in the cells the volume's bounding sphere covers
 * meanwhile, until the next stretch starts beyond the best hit.  With XPBD_SWEEP_BRUTE_FORCE, or for at most
 * XPBD_SWEEP_BRUTE_FORCE_SWEEPS sweeps, every body is looked at instead and no grid is built.  Same bits either way.
 * ------------------------------------------------------------------------- */
#define XPBD_SWEEP_INITIAL 3u             /* xpbd_sweep_hit.feature when the volume overlaps the body at t = 0 */
#define XPBD_SWEEP_BRUTE_FORCE 1u         /* diagnostics: every sweep against every body, no grid */
#define XPBD_SWEEP_MASKED 2u              /* test xpbd_sweep.mask against the bodies' filter groups */
#define XPBD_SWEEP_BRUTE_FORCE_SWEEPS 8u  /* calls with at most this many sweeps take the brute-force path anyway */

typedef struct xpbd_sweep {           /* 104 bytes */
    double   position[3];             /* frame of the volume at t = 0: x_world = position + rotation * x_shape */
    double   rotation[4];             /* {s, x, y, z}, taken as given (the caller keeps it a unit quaternion) */
    double   direction[3];            /* need not be unit; distances are in units of |direction| */
    double   max_distance;            /* may be +inf */
    uint32_t shape;                   /* index into the table of xpbd_world_set_polytopes */
    uint32_t ignore_body;             /* never hit (XPBD_NO_HIT: none) */
    uint32_t mask;                    /* with XPBD_SWEEP_MASKED: body b answers only if (group_b & mask) != 0 */
    uint32_t reserved;                /* must be 0 */
} xpbd_sweep;

typedef struct xpbd_sweep_hit {       /* 72 bytes */
    uint32_t body;                    /* XPBD_NO_HIT: missed */
    uint32_t feature;                 /* XPBD_FEATURE_* (A = the volume, B = the body) or XPBD_SWEEP_INITIAL */
    uint32_t face;                    /* shape-local face of the volume (FACE_A) or the body (FACE_B); else XPBD_NO_HIT */
    uint32_t reserved;                /* 0 */
    double   distance;                /* t */
    double   position[3];             /* sweep.position + t * direction: the volume's frame position at the impact */
    double   normal[3];               /* world space, out of the body towards the volume; (0,0,0) for XPBD_SWEEP_INITIAL */
} xpbd_sweep_hit;

/* Host arrays; checks everything before any device work and waits for the result. */
int  xpbd_world_sweep(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits);
/* Device arrays; stream-ordered on the world's stream, returns before completion (it waits only when its scratch has to
 * grow).  `reserved` is not checked. */
int  xpbd_world_sweep_device(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags,
                             xpbd_sweep_hit *dev_hits);
/* Collective: every rank passes the same sweeps and gets all hits.  Every shard answers for the bodies it OWNS; body and
 * ignore_body are global indices.  Same bits as one xpbd_world over the same bodies. */
int  xpbd_multi_world_sweep(xpbd_multi_world *mw, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags,
                            xpbd_sweep_hit *hits);

/* ---------------------------------------------------------------------------
 * Distance queries (EXTENSION): the body nearest to each of a batch of convex volumes (or points), how far it is, and the two
 * closest points, at the bodies' current poses.  NOT in the reference.  A host asks for proximity sensors, for clearance before
 * a spawn ("5 cm of air around this place", not only "free"), for grasp and placement planning, steering, soft keep-out zones,
 * and to pick the object nearest to a cursor point.
 *
 * The volume of query q is the convex polytope `shape` at the frame fa = {position, rotation}, exactly as for an overlap query.
 * With shape == XPBD_DISTANCE_POINT it is the single point `position`: one vertex (number 0, aw_0 = position itself, no
 * arithmetic), no faces, one edge (number 0, both ends vertex 0), radius 0 and centroid `position`; `rotation` is not used but
 * must still be finite.  Bodies stand at the pose the other queries see.  The ground plane and the terrain are not bodies, and
 * XPBD_QUERY_TERRAIN is an unknown flag for these calls.  (The terrain has calls of its own with the same records:
 * xpbd_world_terrain_distance, "Terrain in the distance queries" below.)
 *
 * One volume A against one body B, with fb = Rigid::frame() of the body.  World vertices aw_v = fa * a_v, bw_v = fb * b_v; in the
 * other's local space a_in_b_v = inverse(fb) * aw_v, b_in_a_v = inverse(fa) * bw_v (the sweep's).  In this order:
 *
 *   1. Overlap.  The pair is "not separated" by exactly rules 2 and 3 of the overlap query -- the tight bounding spheres, then
 *      the decision part of the SAT.  For the point volume: the sphere test with radius_q = 0 and centre `position`, then
 *      max over the faces f of B (face order; the first face's value, replaced by a later one that is larger) of
 *      dot(n_f, a_in_b_0) - disp_f, which must be < 0 (a NaN is not: separated).  A pair that is not separated answers
 *      feature = XPBD_DISTANCE_OVERLAP, distance = 0, index_a = index_b = XPBD_NO_HIT, point_a = point_b = normal = (0,0,0).
 *
 *   2. Otherwise the squared distance d2 is the minimum over the candidates below, visited in this order; the first minimum wins
 *      (a candidate replaces the best so far only if its d2 is strictly smaller; a NaN d2 never is).
 *      The test "x lies in face F of polytope P", for a point x of P's local space, F with the local outward plane (n, disp) and
 *      the vertices w_0 .. w_(m-1) in the face's own winding (face_indices): for k = 0 .. m-1, with a = w_k, b = w_((k+1) % m),
 *      c = w_((k+2) % m):
 *          side = cross(b - a, n);  if dot(side, c - a) > 0 then side = -side;  the edge passes iff dot(side, x - a) <= 0.
 *      x lies in F iff every edge passes (inclusive; a NaN fails).
 *      (a) every vertex v of A (vertex order) against every face f of B (face order), position v * n_faces_b + f, in B's local
 *          space: p = a_in_b_v, h = dot(n, p) - disp.  The candidate counts only if h >= 0 (a NaN: skipped) and foot =
 *          p - h * n (per component: p.x - h * n.x, ...) lies in f.  d2 = h * h.  feature = XPBD_FEATURE_FACE_B, index_a = v,
 *          index_b = f, point_a = aw_v, point_b = fb * foot.
 *      (b) the same with the roles swapped: every vertex v of B against every face f of A, position v * n_faces_a + f, in A's
 *          local space: p = b_in_a_v, h and foot from A's plane, foot in f.  d2 = h * h.  feature = XPBD_FEATURE_FACE_A,
 *          index_a = f, index_b = v, point_a = fa * foot, point_b = bw_v.  The point volume has none of these.
 *      (c) every edge i of A against every edge j of B (edge order), position i * n_edges_b + j, in world space: the clamped
 *          closest points of the segments P0 = aw_(e_i.0), P1 = aw_(e_i.1) and Q0 = bw_(e_j.0), Q1 = bw_(e_j.1).  With
 *          clamp(x) = (x < 0) ? 0 : ((x > 1) ? 1 : x)  (a NaN stays a NaN):
 *              u = P1 - P0, w = Q1 - Q0, r = P0 - Q0, a = dot(u, u), e = dot(w, w), f = dot(w, r);
 *              a == 0 and e == 0:  s = 0, t = 0
 *              a == 0 (e != 0):    s = 0, t = clamp(f / e)
 *              otherwise c = dot(u, r), and
 *                e == 0:           t = 0, s = clamp((-c) / a)
 *                else b = dot(u, w), den = a * e - b * b;  s = (den > 0) ? clamp((b * f - c * e) / den) : 0   (parallel
 *                                  segments, or a denominator that rounding made zero or negative, start from s = 0);
 *                                  t = (b * s + f) / e;
 *                                  t < 0:  t = 0, s = clamp((-c) / a);   else t > 1:  t = 1, s = clamp((b - c) / a)
 *              ca = P0 + u * s, cb = Q0 + w * t (per component), g = ca - cb, d2 = dot(g, g).
 *          feature = XPBD_FEATURE_EDGES, index_a = i, index_b = j, point_a = ca, point_b = cb.  The clamps make this cover
 *          vertex-edge and vertex-vertex, and a vertex whose foot rounding pushed just outside a face.
 *      A pair without any candidate (every d2 a NaN) does not answer.  Then distance = sqrt(d2) and normal = (point_a - point_b)
 *      * (1 / distance) per component, (0,0,0) when distance == 0: it points from the body to the volume.  The candidates are
 *      complete for two disjoint convex polytopes: the closest pair is a vertex over the interior of a face, or two points on
 *      two edges.
 *
 *   3. The pair answers iff distance <= max_distance.
 *
 * Per query the smallest distance wins and equal distances go to the smaller body index (in xpbd_multi_world_distance: the
 * caller's global index).  ignore_body never answers; with XPBD_DISTANCE_MASKED body b answers only if (group_b & mask) != 0
 * (bodies without filters are in group ~0u; without the flag no group is tested).  A body whose pose is not finite never
 * answers.  A query whose `shape` is outside the table and not XPBD_DISTANCE_POINT, whose frame has a NaN or infinite component
 * or whose max_distance is negative or NaN finds nothing (the call still succeeds); max_distance may be +inf.  A miss is
 * {XPBD_NO_HIT, 0, XPBD_NO_HIT, XPBD_NO_HIT, +inf, zeros}.  Quotients and square roots are correctly rounded, there is no fused
 * multiply-add; dot, cross and the frame products are as everywhere else.
 *
 * Errors (host variants, before any device work; the outputs are untouched): XPBD_E_INVALID for a NULL world, NULL queries /
 * hits with n_queries > 0, unknown flags (XPBD_QUERY_TERRAIN included), a nonzero `reserved`, no polytopes set, no bodies
 * resident.  n_queries == 0 is XPBD_OK.  A distance query changes no body, list, mask, report, history entry or plan: stepping
 * after it gives the same bits as stepping without it.  Every mode accepts it.
 *
 * Method: the per-call grid of the ray casts; a group of lanes per query walks the cells its bounding sphere covers, then those
 * the sphere grown by min(max_distance, best so far) covers.  A query that reaches further than a wide sweep's volume may
 * (+inf included) looks at every body.  With XPBD_DISTANCE_BRUTE_FORCE, or for at most XPBD_DISTANCE_BRUTE_FORCE_QUERIES
 * queries, every body is looked at and no grid is built.  Same bits either way.
 * ------------------------------------------------------------------------- */
#define XPBD_DISTANCE_BRUTE_FORCE 1u          /* diagnostics: every query against every body, no grid */
#define XPBD_DISTANCE_MASKED      2u          /* test xpbd_distance_query.mask against the bodies' filter groups */
#define XPBD_DISTANCE_OVERLAP     3u          /* xpbd_distance_hit.feature when the volume and the body are not separated */
#define XPBD_DISTANCE_POINT       0xFFFFFFFFu /* xpbd_distance_query.shape: the volume is the single point `position` */
#define XPBD_DISTANCE_BRUTE_FORCE_QUERIES 8u  /* calls with at most this many queries take the brute-force path anyway */

typedef struct xpbd_distance_query {  /* 80 bytes */
    double   position[3];             /* frame of the volume: x_world = position + rotation * x_shape */
    double   rotation[4];             /* {s, x, y, z}, taken as given (the caller keeps it a unit quaternion) */
    double   max_distance;            /* bodies further away do not answer; may be +inf */
    uint32_t shape;                   /* index into the table of xpbd_world_set_polytopes, or XPBD_DISTANCE_POINT */
    uint32_t ignore_body;             /* never answers (XPBD_NO_HIT: none) */
    uint32_t mask;                    /* with XPBD_DISTANCE_MASKED: body b answers only if (group_b & mask) != 0 */
    uint32_t reserved;                /* must be 0 */
} xpbd_distance_query;

typedef struct xpbd_distance_hit {    /* 96 bytes */
    uint32_t body;                    /* XPBD_NO_HIT: nothing within max_distance */
    uint32_t feature;                 /* XPBD_FEATURE_* (A = the volume, B = the body) or XPBD_DISTANCE_OVERLAP */
    uint32_t index_a;                 /* FACE_B: vertex of the volume; FACE_A: face of the volume; EDGES: edge of the volume */
    uint32_t index_b;                 /* FACE_B: face of the body; FACE_A: vertex of the body; EDGES: edge of the body */
    double   distance;                /* 0 for XPBD_DISTANCE_OVERLAP */
    double   point_a[3];              /* world space, on the volume */
    double   point_b[3];              /* world space, on the body */
    double   normal[3];               /* (point_a - point_b) / distance: from the body to the volume; (0,0,0) at distance 0 */
} xpbd_distance_hit;

/* Host arrays; checks everything before any device work and waits for the result. */
int  xpbd_world_distance(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                         xpbd_distance_hit *hits);
/* Device arrays; stream-ordered on the world's stream, returns before completion (it waits only when its scratch has to
 * grow).  `reserved` is not checked. */
int  xpbd_world_distance_device(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags,
                                xpbd_distance_hit *dev_hits);
/* Collective: every rank passes the same queries and gets all hits.  Every shard answers for the bodies it OWNS; body and
 * ignore_body are global indices.  Same bits as one xpbd_world over the same bodies. */
int  xpbd_multi_world_distance(xpbd_multi_world *mw, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                               xpbd_distance_hit *hits);

/* ---------------------------------------------------------------------------
 * Terrain in the scene queries (EXTENSION): with XPBD_QUERY_TERRAIN in `flags` the heightfield of xpbd_world_set_terrain
 * answers a ray cast, an overlap query and a sweep next to the bodies.  One flag value serves the three families, above each
 * family's own bits.  Accepted by xpbd_world_raycast, _raycast_masked, _raycast_device, _raycast_masked_device,
 * xpbd_world_overlap(_device) and xpbd_world_sweep(_device).  xpbd_multi_world_* has no terrain: there the flag is an unknown
 * flag.  With the flag and no terrain set the call is XPBD_E_INVALID and the outputs are untouched (what
 * xpbd_world_sample_terrain does without a terrain); every other argument check is unchanged, "no polytopes" and "no bodies"
 * included.  Without the flag a call enqueues exactly what it did before: a world with a terrain then answers as one
 * without.  Masks and ignore_body do not concern the terrain: it has no group and no index.  No body has the index
 * XPBD_HIT_TERRAIN: a world holds fewer bodies than that.
 *
 * The terrain as a solid.  With xi = x0 + i * dx and yj = y0 + j * dy (formed exactly so, no fused multiply-add) triangle
 * T = (i, j, k) -- k = 0 the lower triangle of cell (i, j), k = 1 the upper, number 2 * (j * (nx - 1) + i) + k -- stands for
 * the prism under it, unbounded below: the points with
 *     xi <= x <= x(i+1),  yj <= y <= y(j+1),
 *     g = (x - xi) * dy - (y - yj) * dx:  g >= 0 for the lower triangle, g <= 0 for the upper,
 *     dot(n, p) - d <= 0   with {n, d} the plane of T (TERRAIN, steps 4 to 6).
 * The terrain is the union of the prisms, so the ground has an inside.  A query's cell borders are x0 + i * dx; the
 * stepper's lookup puts them where floor((x - x0) / dx) changes.  The two can differ in the last place.
 *
 * One ray (o, dir, max_distance) against T follows the ray-body rule above: t_lo = 0, entering = none, t_hi = max_distance,
 * and the constraints are visited in the order top plane, x slab, y slab, diagonal.
 *   The top plane is (s, v) = (dot(n, o) - d, dot(n, dir)); the diagonal is (g(o), dir.x * dy - dir.y * dx) for the upper
 *   triangle and both negated for the lower (the two triangles of a cell compute the same t bit for bit).  For (s, v):
 *     s or v is NaN: the ray misses;
 *     v < 0: t_k = (-s) / v, and it replaces t_lo only if strictly greater;   v > 0: t_hi = min(t_hi, (-s) / v);
 *     v = 0: the ray misses if s > 0.
 *   A slab [lo, hi] along an axis with components o_a, dir_a:  dir_a = 0: the ray misses unless lo <= o_a <= hi; else
 *     t1 = (lo - o_a) / dir_a, t2 = (hi - o_a) / dir_a; the smaller replaces t_lo if greater, the larger t_hi if smaller.
 *   The ray hits T iff t_lo <= t_hi, at t = t_lo.
 * Neighbouring prisms share the t of their wall and of their diagonal bit for bit, the test t_lo <= t_hi is inclusive and the
 * prisms are solid below, so no ray slips through a seam: where it leaves one prism above that prism's plane it is in the
 * next one from the same t on, and either hits it there (through the wall, if it is already under the next plane) or goes on.
 * The terrain's answer is the minimum over ALL triangles under the order (t, triangle number).  Its fields:
 *   body = XPBD_HIT_TERRAIN;  distance = t;  point = o + t * dir per component;
 *   face = the triangle's number, normal = its n -- also when the ray entered through a wall or the diagonal (a seam of
 *   rounding size, or the outer wall of the field met from outside below the surface);
 *   face = XPBD_RAY_INSIDE and normal = (0,0,0) when nothing entered: the origin is in or under the ground, and t = 0.
 * (A direction component so small that (lo - o_a) / dir_a overflows is still a valid direction: the rule holds as it stands with
 * t = +inf, so such a ray's answer can lie AT t = +inf, distance +inf, as it can for a body.  Every call returns.)
 * A terrain hit's fields do not depend on max_distance, only whether there is one.  A ray that is invalid for the bodies (a
 * NaN or infinite component, a zero direction, a bad max_distance) hits nothing.  The ray's result is the smaller of the
 * bodies' answer and the terrain's under the existing order (t, body): a body wins a tie against the terrain.
 * With XPBD_RAYCAST_BRUTE_FORCE (and XPBD_SWEEP_BRUTE_FORCE) every triangle is tested, a diagnostic for small fields; else the
 * cells under the ray's xy-projection are walked (2D-DDA, every border's t from its own slab expression).  Same bits.
 *
 * Sweeps: vertex against terrain, as the stepper's ground contact.  Every world vertex aw_v = fa * a_v of the volume is the
 * ray (aw_v, direction, max_distance) against the terrain; the winner is the minimum under (t, triangle, vertex).  Fields:
 * body = XPBD_HIT_TERRAIN, feature = XPBD_FEATURE_FACE_B, face = the triangle, normal = n, position = sweep.position +
 * t * direction.  A vertex that starts in or under the ground gives XPBD_SWEEP_INITIAL with t = 0, face = XPBD_NO_HIT and
 * normal = (0,0,0).  The terrain replaces the bodies' hit only if it is strictly earlier.  A sweep that hits no body by
 * its own fields (shape, frame, direction, max_distance; see above) does not hit the terrain either.  As the stepper, this
 * misses a terrain ridge that meets a FACE or an edge of the volume between its vertices.
 *
 * Overlaps: a volume touches the terrain iff the stepper would give it a ground contact there: some vertex x = fq * a_v has
 * the stepper's lookup (TERRAIN, steps 1 to 3) inside the field and s = dot(n, x) - d < 0.  "Free" therefore means "no ground
 * contact in the next step".  The entry is {XPBD_HIT_TERRAIN, XPBD_FEATURE_FACE_B, the smallest s (the first minimum)}: the
 * last of the query's segment, because its index is the largest.  offsets, *n_out and XPBD_E_CAPACITY count it as any other
 * entry.
 * ------------------------------------------------------------------------- */
#define XPBD_QUERY_TERRAIN 0x100u      /* raycast, overlap and sweep flags: the terrain answers too */
#define XPBD_HIT_TERRAIN   0xFFFFFFFEu /* .body of a hit on the terrain */

/* ---------------------------------------------------------------------------
 * Terrain in the distance queries (EXTENSION): the feature of the heightfield's SURFACE nearest to each of a batch of convex
 * volumes or points, how far it is, and the two closest points.  Calls of their own, xpbd_world_terrain_distance(_device),
 * with the records of xpbd_world_distance; that call, its device form and xpbd_multi_world_distance keep refusing
 * XPBD_QUERY_TERRAIN.  The world's nearest thing is the smaller `distance` of the two calls' answers, and a body wins a tie;
 * merging is the caller's.  Hosts ask for hover and foot clearance, "5 cm of air around this spawn place" on a terrain,
 * steering along slopes, the ground point nearest to a cursor or a gripper.  There is no multi-world form: the sharded world has
 * no terrain.  Arithmetic as everywhere: no fused multiply-add, dot / cross / frame products as in the other queries,
 * correctly rounded / and sqrt, and a NaN d2 never replaces anything.
 *
 * The surface.  Sample (i, j) is the point P(i,j) = (x0 + i * dx, y0 + j * dy, H[j][i]), the coordinates formed exactly so, as
 * the ray rule forms its borders; its number is j * nx + i.  Triangle T = (i, j, k) has the number 2 * (j * (nx - 1) + i) + k and
 * the plane {n, d} of the table k_terrain_planes wrote (TERRAIN, steps 4 to 6): every user reads the same bits.  Terrain edge
 * (i, j, e) has the number 3 * (j * nx + i) + e:  e = 0 from P(i,j) to P(i+1,j), it exists iff i < nx - 1;  e = 1 to P(i,j+1),
 * iff j < ny - 1;  e = 2 the diagonal to P(i+1,j+1), iff both.  Every feature of the surface has exactly one number, so shared
 * edges and corners are looked at once.
 *
 * The volume is that of xpbd_world_distance: the polytope `shape` at fa = {position, rotation}, world vertices aw_v = fa * a_v, or
 * the single point `position` for XPBD_DISTANCE_POINT (one vertex, no faces, one edge from vertex 0 to itself).  ignore_body and
 * mask do not concern the terrain and are not read.
 *
 *   1. Not separated: feature = XPBD_DISTANCE_OVERLAP, distance = 0, index_a = index_b = XPBD_NO_HIT, point_a = point_b =
 *      normal = (0,0,0).  The volume is not separated iff (i) or (ii):
 *      (i)  some world vertex x = aw_v (the point volume: `position`) has the stepper's lookup (TERRAIN, steps 1 to 6) inside
 *           the field and s = dot(n, x) - d < 0: exactly the rule by which xpbd_world_overlap with XPBD_QUERY_TERRAIN lists
 *           the terrain;
 *      (ii) polytopes only: some terrain edge hits the volume.  The edge Q0 Q1 is the ray (origin = Q0, direction = Q1 - Q0,
 *           max_distance = 1), the volume a body with frame fa, the test the ray-body rule above: hit iff t_lo <= t_hi.  This
 *           catches the ridge or peak that pokes into a face or an edge of the volume between its vertices; a terrain vertex
 *           inside the volume is the start or the end of such an edge and needs no rule of its own.
 *   2. Otherwise d2 is the minimum over the candidates below under the total order (d2, class, terrain feature number, the
 *      volume's index), class (a) < (b) < (c): the first minimum of the literal loop "all of (a), then all of (b), then all of
 *      (c), terrain feature ascending, the volume's index ascending within it" (a candidate replaces the best so far only if
 *      its d2 is strictly smaller).  The order is total, so which features an implementation looks at cannot change a bit.
 *      (a) every volume vertex p = aw_v against every triangle T, in world space: h = dot(n, p) - d, counted only if h >= 0;
 *          foot = p - h * n per component, which must satisfy the xy constraints of T's prism, inclusive, a NaN failing:
 *          xi <= foot.x <= x(i+1), yj <= foot.y <= y(j+1), g = (foot.x - xi) * dy - (foot.y - yj) * dx with g >= 0 for the
 *          lower triangle and g <= 0 for the upper.  d2 = h * h, feature = XPBD_FEATURE_FACE_B, index_a = v, index_b = the
 *          triangle's number, point_a = p, point_b = foot.
 *      (b) polytopes only: every sample P against every face f of the volume, in the volume's local space: p = inverse(fa) * P
 *          and rule 2 (b) of the distance queries as it stands (h >= 0, the foot in f by the face's own winding test).
 *          d2 = h * h, XPBD_FEATURE_FACE_A, index_a = f, index_b = the sample's number, point_a = fa * foot, point_b = P.
 *      (c) every edge of the volume (the point: its one edge) against every terrain edge, in world space: the clamped segment
 *          rule 2 (c) of the distance queries, branch by branch, with P0 P1 the volume's edge and Q0 Q1 the terrain's.
 *          XPBD_FEATURE_EDGES, index_a = the volume's edge, index_b = the terrain edge's number, point_a = ca, point_b = cb.
 *      Then distance = sqrt(d2) and normal = (point_a - point_b) * (1 / distance) per component, (0,0,0) at distance 0: it
 *      points from the ground to the volume.
 *   3. The terrain answers iff distance <= max_distance, with body = XPBD_HIT_TERRAIN; else the distance queries' miss record.
 *      A query whose shape is outside the table and not the point, whose frame is not finite or whose max_distance is negative
 *      or NaN finds nothing, and the call still succeeds.
 *
 * What this is and is not.  Above the field the candidates are complete for a volume that rules (i) and (ii) call separated:
 * the closest pair is a vertex over the interior of a triangle, a sample over the interior of a face, or two points on two
 * edges, clamps included.  Beyond the field's border there is no ground, as for the stepper: a vertex outside the field cannot
 * make rule (i) true, and the nearest feature may then be a border edge.  A volume wholly inside the solid is OVERLAP through
 * (i).  Not caught: a volume that skewers a hill -- in through one triangle's interior, under the ridge edge, out through the
 * next triangle's, both ends in the air -- has no vertex under the ground and meets no terrain edge; the rules call it separated.
 *
 * Flags: XPBD_DISTANCE_BRUTE_FORCE -- every sample is looked at, a diagnostic for small fields -- and XPBD_DISTANCE_MASKED,
 * accepted and ignored so that a caller can pass the flags of its body call.  Everything else is unknown, XPBD_QUERY_TERRAIN
 * included.  XPBD_E_INVALID, the outputs untouched: a NULL world, NULL queries / hits with n_queries > 0, unknown flags, a
 * nonzero `reserved` (host variant only), a world without a terrain (xpbd_world_set_terrain).  n_queries == 0 is XPBD_OK.
 * Neither bodies nor polytopes are required: without polytopes the shape table is empty and only point queries find anything.
 * The call changes nothing: stepping after it gives the bits of stepping without it.
 *
 * Method: a group of lanes per query visits rings of samples around the one under the volume's centre and stops when the ring's
 * inner border is further from the volume's bounding sphere than min(max_distance, best so far).  Same bits as brute force.
 * ------------------------------------------------------------------------- */
/* Host arrays; checks everything before any device work and waits for the result. */
int  xpbd_world_terrain_distance(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                                 xpbd_distance_hit *hits);
/* Device arrays; stream-ordered on the world's stream, returns at once: it has no scratch of its own and never waits.
 * `reserved` is not checked. */
int  xpbd_world_terrain_distance_device(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags,
                                        xpbd_distance_hit *dev_hits);

/* ---------------------------------------------------------------------------
 * Contact REPORTS (EXTENSION): which body pairs the contact pipeline of XPBD_MODE_CONTACTS found touching, with the
 * manifolds it solved, and which pairs began or ended touching.  NOT in the reference; its app draws the reference and
 * incident planes of `sat` into DebugLines (src/collision.rs:69, 87) and, commented out, the contact points (:97-108).
 *
 * Frame.  A frame runs from one broadphase (xpbd_world_step, xpbd_world_contacts_begin, xpbd_world_build_neighbours) to
 * the next one.  The report describes the current frame once at least one of its substeps has run; with the split API a
 * download mid-frame covers the substeps run so far.
 *
 * Touching.  A pair touches in a substep when its manifold of that substep has n_points > 0.  Pairs the sphere pre-test
 * answers, GJK's degenerate queries and separated pairs do not touch.  Filtered pairs (xpbd_world_set_collision_filters)
 * are never reported: they are not in the pair list.
 *
 * Pair records: every pair that touched in at least one substep of the frame, sorted by (body_a, body_b), body_a <
 * body_b, the caller's body indices.  `substeps` = the substeps of the frame in which it touched; the rest describes the
 * LAST substep, as the pair solve used it -- the points at the post-integrate poses P1 (oracle/xpbd_pairs_oracle.h,
 * step 2):
 *   n_points  0 when the pair touched only in earlier substeps (then feature = 0, normal = (0,0,0), depth = 0);
 *   feature   XPBD_FEATURE_*;
 *   points    p_ref[k] on the reference body, p_inc[k] the incident body's penetrating point.  A face contact's p_ref[k] is
 *             p_inc[k] projected onto the reference plane with the clipper's own expression,
 *             p_inc - (dot(n, p_inc) - d) * n  (Plane::project, src/geometry.rs:45-47), so it equals the oracle's bits;
 *   normal    from body_a towards body_b: a face contact's reference-plane normal, negated for XPBD_FEATURE_FACE_B; the
 *             one-point contact (XPBD_FEATURE_EDGES: edges, or GJK + EPA without a face normal): u * (1 / |u|) with
 *             u = p_ref[0] - p_inc[0], (0,0,0) when u is zero;
 *   depth     max over k of |p_ref[k] - p_inc[k]|.
 * `first_point` indexes the point list, in which every pair's points follow each other in pair order.
 *
 * Events.  With S the touching set of this frame and S_prev the one of the world's previous frame: XPBD_CONTACT_BEGIN for
 * every pair of S not in S_prev, XPBD_CONTACT_END for every pair of S_prev not in S; all BEGINs in key order, then all
 * ENDs in key order.  S_prev is EMPTY after enabling reports, after xpbd_world_upload_bodies,
 * after xpbd_world_history_restore, after a step in another mode and after a failed step.  After a failed step or a step
 * in another mode, and until the next broadphase of XPBD_MODE_CONTACTS has run a substep, the counts and downloads are
 * XPBD_E_INVALID.  Joints, limits, filters, the narrowphase and the SAT schedule may change between frames.
 *
 * The report only reads: bodies, contact lists, masks, statistics and history are the same bits with reporting on or off,
 * and with reporting off (the default) no part of it runs.
 *
 * Calls.  xpbd_world_set_contact_report: enable 0 or 1, in any mode (only steps in XPBD_MODE_CONTACTS produce a report).
 * The counts and downloads wait for the device.  Capacities as xpbd_world_download_contacts: the totals always go to
 * *n_pairs / *n_points / *n_out, a short buffer gets XPBD_E_CAPACITY with its first `cap` entries filled.  points == NULL
 * (with point_cap 0) downloads no points and is no capacity error.  XPBD_E_INVALID: a NULL world, reporting off, no report
 * available (above), NULL counts, or a NULL buffer with a nonzero capacity.
 *
 * Multi world (xpbd_multi_world_*): the same report with global body indices, the same bits as one xpbd_world over the same
 * bodies, events included.  Every shard reports the pairs whose lower body it owns; xpbd_multi_world_step (collective) gathers
 * the lists of all ranks at the end of every accepted frame and merges them, so every rank holds the whole world's report and
 * derives the events from the merged lists (owners changing at a re-plan do not matter; a frame that is undone and re-run under
 * XPBD_MULTI_AUTO_REPLAN leaves no trace).  The counts and downloads then read that copy: they communicate nothing and may be
 * called on any rank.  S_prev is empty after enabling, after xpbd_multi_world_upload and after a failed step.
 * ------------------------------------------------------------------------- */
#define XPBD_CONTACT_BEGIN 0u
#define XPBD_CONTACT_END   1u

typedef struct xpbd_pair_contact {   /* 64 bytes */
    uint32_t body_a, body_b;         /* body_a < body_b */
    uint32_t substeps;               /* substeps of the frame in which the pair touched (>= 1) */
    uint32_t n_points;               /* in the last substep (0: touched only earlier in the frame) */
    uint32_t feature;                /* XPBD_FEATURE_* of the last substep (valid when n_points > 0) */
    uint32_t first_point;            /* index of its first point in the point list */
    uint32_t reserved[2];
    double   normal[3];
    double   depth;
} xpbd_pair_contact;

typedef struct xpbd_contact_point {  /* 48 bytes, world space, last substep */
    double p_ref[3];                 /* on the reference body's surface */
    double p_inc[3];                 /* the penetrating point of the incident body */
} xpbd_contact_point;

typedef struct xpbd_contact_event {  /* 12 bytes */
    uint32_t body_a, body_b, kind;   /* XPBD_CONTACT_* */
} xpbd_contact_event;

int  xpbd_world_set_contact_report(xpbd_world *w, uint32_t enable);
/* out = {pairs, points, begins, ends} */
int  xpbd_world_contact_report_counts(xpbd_world *w, uint32_t out[4]);
int  xpbd_world_download_pair_contacts(xpbd_world *w, xpbd_pair_contact *pairs, uint32_t pair_cap,
                                       xpbd_contact_point *points, uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points);
int  xpbd_world_download_contact_events(xpbd_world *w, xpbd_contact_event *out, uint32_t cap, uint32_t *n_out);
int  xpbd_multi_world_set_contact_report(xpbd_multi_world *mw, uint32_t enable);
int  xpbd_multi_world_contact_report_counts(xpbd_multi_world *mw, uint32_t out[4]);
int  xpbd_multi_world_download_pair_contacts(xpbd_multi_world *mw, xpbd_pair_contact *pairs, uint32_t pair_cap,
                                             xpbd_contact_point *points, uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points);
int  xpbd_multi_world_download_contact_events(xpbd_multi_world *mw, xpbd_contact_event *out, uint32_t cap, uint32_t *n_out);

/* ---------------------------------------------------------------------------
 * Contact ISLANDS (EXTENSION): which bodies belong together -- a pile, a jointed mechanism, a stack on a slab -- what holds
 * each group up, and whether it has stopped moving.  NOT in the reference, whose world is a fixed pair of `Rigid`s
 * (src/world.rs).  One connected-components pass on the device over what is already resident there: the contact report's
 * touching pairs, the joints, the mass properties, the velocities and the last substep's ground contacts.
 *
 * Fixed body.  A body is fixed when inverse_mass == 0 and all nine inverse_inertia entries are == 0.  A body with zero
 * inverse mass but a nonzero inverse inertia can still turn: it is not fixed.
 *
 * Graph.  The nodes are the non-fixed bodies.  The edges are (a) every pair of the current report frame's touching set S
 * ("Contact REPORTS" above: the pairs the BEGIN / END events use, those that touched in at least one substep of the frame)
 * and (b) every joint of the world, of any kind.  An edge with ONE fixed end connects nothing; it is counted as an anchor
 * of its other end's island (otherwise everything resting on one slab would be a single island).  An edge between two fixed
 * bodies is ignored.
 *
 * Island.  One connected component; a non-fixed body without edges is an island of one.  Islands are numbered 0..K-1 in
 * ascending order of their smallest member.  The numbering, like everything else the calls return, does not depend on
 * scheduling: the grouping keeps the smallest member as the root of every component, the numbers come from a scan, and the
 * records are integer sums and integer maxima.
 *
 * Records.  island_of[i] is the island of body i, XPBD_ISLAND_NONE for a fixed body.  Per island:
 *   first_body          its smallest member;
 *   n_bodies            its members;
 *   n_pairs, n_joints   touching pairs / joints with both ends in the island (the same two bodies joined twice count twice);
 *   n_anchors           touching pairs and joints between a member and a fixed body;
 *   n_grounded          members whose LAST substep had a ground contact (plane or terrain): the contact mask as it stands,
 *                       so zero after an upload or a population change, and what the history restored after a restore;
 *   max_speed2          the largest v.x * v.x + v.y * v.y + v.z * v.z (evaluated left to right) over the members' velocity,
 *   max_angular_speed2  the same of angular_velocity.  Both maxima are taken over the BIT PATTERNS of the values with the
 *                       sign bit cleared, compared as unsigned 64-bit integers: order-free, exact, and a NaN shows as a NaN.
 * With XPBD_ISLANDS_NO_JOINTS the edges (b), with XPBD_ISLANDS_NO_CONTACTS the edges (a) count NOWHERE: they add neither
 * connectivity nor n_pairs / n_joints / n_anchors.  XPBD_ISLANDS_NO_CONTACTS needs no contact report.
 *
 * Calls.  xpbd_world_islands takes host arrays and waits for the device.  It always writes the island count to *n_islands
 * and fills min(count, cap) records; a count above cap is XPBD_E_CAPACITY, as xpbd_world_download_contacts.  islands == NULL
 * with cap == 0 and island_of == NULL are allowed.  xpbd_world_islands_device takes DEVICE arrays (8-byte aligned records)
 * and only enqueues on the world's stream (xpbd_world_get_stream / _set_stream): no wait, no host read, the number of
 * touching pairs is read on the device; it writes the count to *dev_n_islands and only the first `cap` records.  (The
 * unit's scratch grows on the first call and when the body or pair count has grown: only then does the call wait for the
 * stream, as every stream-ordered call of the library.)  Its flags compose with xpbd_world_remove_bodies_device.
 *
 * The grouping is lock-free and every loop of it is bounded by construction; the bound is carried anyway.  Should a lane
 * reach it, xpbd_world_islands returns XPBD_E_HIP and xpbd_world_islands_device leaves XPBD_ISLAND_NONE in *dev_n_islands.
 *
 * XPBD_E_INVALID, nothing written: a NULL world or count; a NULL record buffer with a nonzero cap; unknown flag bits; both
 * flags together; a world without resident bodies; and, without XPBD_ISLANDS_NO_CONTACTS, exactly when
 * xpbd_world_contact_report_counts is XPBD_E_INVALID (reporting off, no report frame: "Contact REPORTS").
 *
 * The calls only read: bodies, report downloads, events, history and every later step are the same bits whether or not they
 * were made, and a world that never makes them enqueues nothing new.
 *
 * Not here: the multi-GPU world (xpbd_multi_world_*).  Its report lives merged on the host and its bodies on several
 * devices; islands there are a different design.  These calls cover the single world only.
 * ------------------------------------------------------------------------- */
#define XPBD_ISLAND_NONE         0xFFFFFFFFu /* island_of[] of a fixed body */
#define XPBD_ISLANDS_NO_JOINTS   1u          /* edges (a) only */
#define XPBD_ISLANDS_NO_CONTACTS 2u          /* edges (b) only; needs no contact report */

typedef struct xpbd_island {     /* 40 bytes */
    uint32_t first_body;         /* smallest member */
    uint32_t n_bodies;
    uint32_t n_pairs;            /* touching pairs with both bodies in the island */
    uint32_t n_joints;           /* joints with both ends in the island */
    uint32_t n_anchors;          /* touching pairs and joints between a member and a fixed body */
    uint32_t n_grounded;         /* members whose last substep had a ground (plane or terrain) contact */
    double   max_speed2;         /* max over members of v.x*v.x + v.y*v.y + v.z*v.z, left to right */
    double   max_angular_speed2; /* the same of angular_velocity */
} xpbd_island;

int  xpbd_world_islands(xpbd_world *w, uint32_t flags, uint32_t *island_of /* [body count] or NULL */,
                        xpbd_island *islands, uint32_t cap, uint32_t *n_islands);
int  xpbd_world_islands_device(xpbd_world *w, uint32_t flags, uint32_t *dev_island_of /* or NULL */,
                               xpbd_island *dev_islands, uint32_t cap, uint32_t *dev_n_islands);

/* ---------------------------------------------------------------------------
 * SLEEPING (EXTENSION): resting groups of bodies leave the step until something disturbs them.  NOT in the reference.  Opt-in:
 * a world that never calls xpbd_world_set_sleeping runs exactly what it ran before.  Single world, XPBD_MODE_CONTACTS, contact
 * report on (the touching set is the report's S, "Contact REPORTS").
 *
 * Per body the world keeps  asleep (0 / 1),  rest_frames (consecutive frames at rest)  and  group (the smallest member of the
 * island the body fell asleep with; XPBD_SLEEP_GROUP_NONE while awake).  Enabling starts every body awake with rest_frames 0.
 *
 * Fixed body and island: exactly as in "Contact ISLANDS" above.  INERT: asleep or fixed.
 *
 * At rest.  A body is at rest when  v.x*v.x + v.y*v.y + v.z*v.z <= linear_speed*linear_speed  for its velocity and the same
 * expression of its angular_velocity is <= angular_speed*angular_speed; every expression evaluated left to right without
 * contraction, as max_speed2 of the islands is.  A NaN compares false: not at rest.
 *
 * During a frame (one xpbd_world_step) the asleep set does not change, and
 *  (a) the broadphase forms no pair whose two ends are both inert.  The pair list, xpbd_world_contact_stats and the report
 *      change with it: the report holds only pairs with at least one awake, non-fixed body; the pairs inside a group that falls
 *      asleep produce END events in the next frame, those of a group that wakes BEGIN events;
 *  (b) no per-body stage advances an asleep body -- integrate + ground, pair solve, derive, restitution: its 13 dynamic
 *      doubles, its contact mask (xpbd_world_download_contacts; the trace rows of a step repeat it) stay the same bits;
 *  (c) awake neighbours see an asleep body through a body record made from its resting pose: frame before integrate = frame
 *      after integrate = Rigid::frame(), pose after the ground contacts = its pose, with its own mass properties.  (A
 *      neighbour's correction is therefore shared as with an awake body, but the sleeper's share is not applied in that frame.)
 *      Friction's past frame of a sleeper is that same Rigid::frame(), so its contact points have no travel of their own.  Stage 6
 *      (RESTITUTION) reads a sleeper's v0, w0 and its v, w after derive as the +0.0 that step 3 below stored -- every edit of
 *      a sleeper wakes it before the next step, so no sleeper carries another value -- shares the impulse with the sleeper's own
 *      W, and drops the sleeper's entry as the position pass drops its share.  The ground contact mask a sleeper keeps is its
 *      own: it enters no neighbour's count.
 *
 * The sleep pass runs at the end of every xpbd_world_step, on the state the last substep left, in this order:
 *  1. Wake.  Every asleep body s is MARKED when the frame's touching set holds a pair (s, a) with a awake and not fixed.  Every
 *     asleep body whose group equals the group of a marked body wakes: asleep = 0, rest_frames = 0, group = NONE.
 *  2. Count.  For every body that is now awake and not fixed:  rest_frames = at rest ? min(rest_frames + 1, UINT32_MAX) : 0.
 *  3. Sleep.  Take the islands of the frame as xpbd_world_islands(flags 0) returns them.  An island none of whose members is
 *     asleep and all of whose members have rest_frames >= frames_to_sleep goes to sleep: asleep = 1, group = the island's
 *     first_body, velocity and angular_velocity = +0.0 for every member.  rest_frames keeps its value.  (The grouping is the
 *     islands call's, loop bound included: should a lane ever reach the bound -- the case in which xpbd_world_islands returns
 *     XPBD_E_HIP -- the pass puts nobody to sleep in that frame, counts[3] is 0, and steps 1 and 2 stand.  The step itself does
 *     not fail: nothing waits for the device.)
 * counts[2] / counts[3] of xpbd_world_sleep_state are the bodies step 1 woke / step 3 put to sleep in the last pass.
 *
 * Wake requests between frames are applied by the same group-wide wake at the START of the next xpbd_world_step, before its
 * broadphase (until then xpbd_world_sleep_state shows the state the last pass left):
 *   xpbd_world_wake_bodies(_device): the groups of the listed sleepers; indices == NULL with n == 0: everybody.
 *   xpbd_world_set_external_wrench(_device), xpbd_world_apply_impulses(_device), xpbd_world_set_dynamics: the groups of the
 *     sleepers they name.  A call that names a FIXED body wakes everybody (an anchor may have moved).  An awake body keeps
 *     its rest_frames.  (The edit itself is applied at once, to a sleeper too.)
 *   xpbd_world_set_joints, _set_joint_limits, _set_joint_drives, _set_collision_filters, _set_materials, _set_restitution,
 *     _set_terrain, _set_polytopes, _set_contact_pad: everybody wakes and every rest_frames becomes 0.
 *   xpbd_world_upload_bodies and a population change (xpbd_world_add_bodies, _remove_bodies that removes a body): the state
 *     starts over at once, every body awake with rest_frames 0; sleeping stays on.
 * The device variants scatter their requests on the device and wait for nothing; an index outside the world is skipped.
 *
 * Kinematic bodies ("KINEMATIC bodies").  An entry's body is MOVING in a frame when, at the frame's start, its mode is POSE and
 * the overwrite before the first substep produced any nonzero velocity or angular-velocity component, or its mode is VELOCITY
 * and any of its six components is nonzero.  With sleeping on,
 *   - a MOVING body is not inert in that frame: inert = asleep || (fixed && !moving), so the broadphase forms its pairs with
 *     sleepers (rule (a) reads "inert" so);
 *   - wake step 1 additionally MARKS every asleep body that shares a pair of the frame's PAIR LIST (the broadphase's, not the
 *     touching set: a platform that moves away from a resting stack stops touching it in the first substep, and a floater must
 *     never be left behind) or a joint with a MOVING body.  The rule is conservative: a sleeper whose bounding sphere the
 *     moving body's swept sphere merely passes wakes too, and sleeps again once it has rested;
 *   - for the islands a kinematic body remains a fixed body: an anchor, never a member; it never sleeps and has no counter.
 * The sleepers stay asleep DURING the frame in which the body first moves (the asleep set does not change within a frame): they
 * follow from the next frame on.  xpbd_world_set_kinematic_targets(_device) and xpbd_world_set_kinematics request no wake by
 * themselves -- only motion does, and only near the body that moves; xpbd_world_set_dynamics on a fixed body still wakes
 * everybody.  A world with sleeping on and an empty kinematic table launches the sleeping kernels it launched before.
 *
 * History.  While sleeping is on an entry carries asleep, rest_frames, group and the pending requests, and a restore brings
 * them back: a run repeated from a restored entry is the same bits, sleep state included.  Turning sleeping on or off changes
 * the size of an entry, so both drop the history (xpbd_world_history_length becomes 0).
 *
 * xpbd_world_set_sleeping(w, cfg) turns sleeping on or, when already on, replaces the configuration and keeps the state;
 * cfg == NULL turns it off: everything is awake, and the world steps as a world that never slept given its bodies.
 * XPBD_E_INVALID, nothing changed: a NULL world; a negative or non-finite speed; frames_to_sleep == 0; flags != 0; a mode other
 * than XPBD_MODE_CONTACTS; the contact report off.  While sleeping is on, xpbd_world_set_contact_report(w, 0),
 * xpbd_world_set_mode to another mode, the split API (xpbd_world_contacts_begin / _substep: it has no frame end) and the
 * diagnostic xpbd_world_build_neighbours (a broadphase outside a step: it would have to apply the wake requests early) are
 * XPBD_E_INVALID.
 *
 * xpbd_world_sleep_state takes host arrays of the body count (any may be NULL) and waits; counts = {asleep bodies, sleeping
 * groups, bodies woken by the last pass, bodies put to sleep by it}.  xpbd_world_sleep_state_device takes device arrays and
 * only enqueues on the world's stream.  Both, and the wake calls, are XPBD_E_INVALID when sleeping is off; the host variant
 * of the wake call also for NULL indices with n != 0 and for an index >= the body count (nothing is requested then).
 *
 * Not here: the multi-GPU world; putting bodies to sleep by request; keeping sleepers asleep across a population change.
 * And by decision no wake from xpbd_world_set_shapes, xpbd_world_set_narrowphase, xpbd_world_set_sat_schedule and
 * xpbd_world_set_max_depenetration_speed: they change how a step computes, not what a resting group rests on.  Sleepers stay
 * asleep across them; a caller who wants otherwise calls xpbd_world_wake_bodies(w, NULL, 0).
 * ------------------------------------------------------------------------- */
typedef struct xpbd_sleep_config {   /* 24 bytes */
    double   linear_speed;           /* m/s, finite, >= 0 */
    double   angular_speed;          /* rad/s, finite, >= 0 */
    uint32_t frames_to_sleep;        /* >= 1: consecutive frames at rest before an island may sleep */
    uint32_t flags;                  /* 0 */
} xpbd_sleep_config;
#define XPBD_SLEEP_GROUP_NONE 0xFFFFFFFFu /* group[] of a body that is awake */

int  xpbd_world_set_sleeping(xpbd_world *w, const xpbd_sleep_config *cfg /* NULL: off */);
int  xpbd_world_sleep_state(xpbd_world *w, uint8_t *asleep, uint32_t *rest_frames, uint32_t *group, uint32_t counts[4]);
int  xpbd_world_sleep_state_device(xpbd_world *w, uint8_t *dev_asleep, uint32_t *dev_rest_frames, uint32_t *dev_group,
                                   uint32_t *dev_counts /* [4] */);
int  xpbd_world_wake_bodies(xpbd_world *w, const uint32_t *indices, uint32_t n /* NULL, 0: all */);
int  xpbd_world_wake_bodies_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n /* NULL, 0: all */);

/* ---------------------------------------------------------------------------
 * SENSOR bodies (EXTENSION): triggers -- bodies that see what enters them and push nothing: goal zones, pressure plates,
 * pick-up volumes, a proximity zone carried by a kinematic gripper.  NOT in the reference.  Opt-in: a world whose sensor table is
 * empty or all zero enqueues exactly what it enqueued before.  Single world, XPBD_MODE_CONTACTS.
 *
 * Definition.  A SENSOR is a body whose byte in the per-body table of xpbd_world_set_sensors is 1.  A SENSOR PAIR is a pair of
 * the frame's pair list with at least one sensor end.  Only body-body pairs are affected: a dynamic sensor still integrates, hits
 * the ground or the terrain, obeys joints, drives, damping and kinematic scripts, and is hit by the scene queries.  A fixed or
 * kinematic sensor is the usual trigger.
 *
 * Never solved.  A sensor pair is still formed by the broadphase, subject to the collision filters as they are: group and mask
 * bits are how a caller makes a sensor selective.  Its narrowphase runs every substep and its manifold and code are written as
 * for any pair.  But the pair solve (both of its forms), the restitution pass and the depenetration limit see a code of 0 for
 * it: no contact.  Every body of a world with sensors therefore steps BIT FOR BIT like the same world in which the sensor bodies
 * carry the filter {group 0, mask 0} and no sensor flag.  The touching-pair and point counts of xpbd_world_contact_stats, which
 * are counted inside the pair solve (and from which the SAT schedule is chosen), exclude sensor pairs; its pair count includes
 * them.
 *
 * Reported.  The contact report ("Contact REPORTS") treats a sensor pair like any pair, with no special case: its touching
 * substeps, the last substep's feature, normal, depth and points at the post-integrate poses, and BEGIN / END against the
 * previous frame.  Sensor-sensor pairs are reported too.
 *
 * Islands and sleeping.  Sensor pairs are not contact edges ("Contact ISLANDS"): they add no connectivity, n_pairs or
 * n_anchors, and wake step 1 of the sleep pass ("SLEEPING") does not read them: they wake nobody.  With sleeping on a sensor is
 * never inert for the broadphase (inert = 0 for it, whatever it is), so a body that falls asleep inside a fixed sensor keeps its
 * pair: no END event at sleep, and it is still listed by the occupancy below.  The wake rule of a MOVING kinematic body is
 * unchanged -- it reads the frame's pair list, not the touching set -- so a MOVING kinematic sensor wakes what it shares a pair
 * with.
 *
 * Lifetime.  xpbd_world_upload_bodies clears the table.  xpbd_world_remove_bodies / _add_bodies carry each survivor's flag; new
 * bodies are not sensors.  History push and restore do not carry the table.  Setting or clearing the table while sleeping is on
 * wakes everybody and zeroes every rest_frames, as the other table setters do.
 *
 * xpbd_world_set_sensors(w, is_sensor, n) replaces the table: n == the body count, one byte per body; NULL with n == 0 clears
 * it.  XPBD_E_INVALID, the previous table left in force: a NULL world; NULL with n > 0; n different from the body count; a byte
 * other than 0 or 1 (the other bits stay reserved).  xpbd_world_get_sensors writes the table as it stands (all 0 without one);
 * XPBD_E_INVALID for a NULL world, NULL with n > 0, n different from the body count.  xpbd_world_sensor_count: the bodies
 * flagged (0 for a NULL world).
 *
 * Occupancy.  xpbd_world_sensor_overlaps answers, for the current report frame: sensors[k] = the k-th sensor in ascending body
 * index (k < xpbd_world_sensor_count), and hits[offsets[k] .. offsets[k + 1]) = the bodies that touched it in at least one
 * substep of the frame, ascending by body, each with the index of the pair's record in xpbd_world_download_pair_contacts.  A
 * pair of two sensors is listed under both.  The host variant takes host arrays (sensors: sensor count entries, offsets: one
 * more) and waits for the device; the capacity rule is that of xpbd_world_overlap: offsets are always complete, *n_out is the
 * total, and with more than `cap` hits XPBD_E_CAPACITY is returned with the first `cap` filled.  xpbd_world_sensor_overlaps_device
 * takes DEVICE arrays, only enqueues on the world's stream (it waits only when its scratch has to grow) and writes only the
 * first `cap` hits, the total being dev_offsets[sensor count]; it composes with xpbd_world_joint_states_device,
 * xpbd_world_set_drive_targets_device and xpbd_world_set_kinematic_targets_device, so a loop "who is in the zone -> retarget"
 * never leaves the device.  No atomic and no sort decide an order: the lists do not depend on the schedule.  XPBD_E_INVALID,
 * nothing written: a NULL world; a NULL sensors or offsets array, a NULL hits array with a nonzero cap, for the host variant a
 * NULL n_out; no sensor set; and exactly when xpbd_world_contact_report_counts is XPBD_E_INVALID (reporting off, no report
 * frame).  The calls only read.
 *
 * Not here: the multi-GPU world (xpbd_multi_world_*); a per-sensor filter beyond group / mask.
 * ------------------------------------------------------------------------- */
typedef struct xpbd_sensor_hit {   /* 8 bytes */
    uint32_t body;                 /* the other body of a touching sensor pair */
    uint32_t pair;                 /* index of the pair's record in xpbd_world_download_pair_contacts */
} xpbd_sensor_hit;

int      xpbd_world_set_sensors(xpbd_world *w, const uint8_t *is_sensor, uint32_t n /* == body count; NULL, 0: clear */);
int      xpbd_world_get_sensors(xpbd_world *w, uint8_t *is_sensor, uint32_t n);
uint32_t xpbd_world_sensor_count(const xpbd_world *w) XPBD_NOEXCEPT;
int      xpbd_world_sensor_overlaps(xpbd_world *w, uint32_t *sensors, uint32_t *offsets, xpbd_sensor_hit *hits, uint32_t cap,
                                    uint32_t *n_out);
int      xpbd_world_sensor_overlaps_device(xpbd_world *w, uint32_t *dev_sensors, uint32_t *dev_offsets, xpbd_sensor_hit *dev_hits,
                                           uint32_t cap);

/* Diagnostics: quotient[i] = a[i] / b[i], root[i] = sqrt(a[i]) computed on the
 * device with the stepper's own code generation.  Bit-exact contact lists need
 * both to be correctly rounded; the parity tests check this against the host. */
int  xpbd_selftest_div_sqrt(int32_t device, const double *a, const double *b,
                            double *quotient, double *root, uint32_t n);
/* Diagnostics: the stepper's two short sequences (xpbd_exact.hpp) next to the plain expressions, all evaluated on the device.
 * fast[0..n) = div_by(x[i], h), fast[n..2n) = s and fast[2n..3n) = k of sqrt_and_reciprocal(a[i]);
 * plain[0..n) = x[i] / h, plain[n..2n) = sqrt(a[i]), plain[2n..3n) = 1.0 / sqrt(a[i]).  The two must agree bit for bit. */
int  xpbd_selftest_exact_math(int32_t device, const double *x, const double *a, double h, uint32_t n,
                              double *fast /* [3n] */, double *plain /* [3n] */);

/* Diagnostics: the HBM roof as this library can reach it -- a device-to-device copy of `bytes` (use far more than the
 * 256 MiB Infinity Cache) by the library's own streaming kernel, `repeats` launches timed with HIP events.
 * *gbytes_per_s = (bytes read + bytes written) / time, in 1e9 bytes per second. */
int  xpbd_selftest_hbm_copy(int32_t device, uint64_t bytes, uint32_t repeats, double *gbytes_per_s);
/* Diagnostics: what the memory system gives the ACCESS PATTERN of one substep of the pinned path -- 38 doubles read and 13
 * written per body and nothing else -- in the world's field-major layout (tile_major = 0: 51 concurrent streams of 512
 * bytes per wave) or tile-major (1: 64 bodies x all fields contiguous); best of `repeats` launches.  This, not the
 * two-stream copy above, is the roof of XPBD_MODE_PER_SUBSTEP on worlds beyond the Infinity Cache. */
int  xpbd_selftest_field_streams(int32_t device, uint64_t bodies, uint32_t tile_major, uint32_t repeats, double *gbytes_per_s);

/* Diagnostics: a GATHER of known size -- lane i reads the first read_bytes of record perm(i) of `records` records (a power of
 * two) of record_bytes each with 16-byte loads, every record exactly once, and writes one double; (read_bytes, record_bytes)
 * one of (128, 128), (64, 128), (16, 128), (192, 192), (64, 192), (128, 256): how the contact kernels read body records, mass
 * properties and manifolds.  *gbytes_per_s = (records * read_bytes + records * 8) / best time.  Under `rocprofv3 --pmc
 * FETCH_SIZE` this calibrates the counter for gathered loads (profiles/, scripts/fetch_calibration.py). */
int  xpbd_selftest_gather(int32_t device, uint32_t records, uint32_t record_bytes, uint32_t read_bytes, uint32_t repeats,
                          double *gbytes_per_s);

#ifdef __cplusplus
}
#endif
#endif /* XPBD_H */
