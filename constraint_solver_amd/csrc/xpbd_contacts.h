// xpbd_contacts.h -- body-body contact EXTENSION: broadphase + per-substep contact pipeline.
// Semantics are defined by oracle/xpbd_pairs_oracle.h (op_contacts_step); parity unpinned.
// The structs, and the launchers of xpbd_broadphase.hip, xpbd_contacts.hip, xpbd_restitution.hip and xpbd_terrain.hip.
#pragma once

#include "xpbd_pairs.h"

namespace xpbd {

// xpbd_joint, device copy.
struct Joint {
    uint32_t body_a, body_b;
    double anchor_a[3], anchor_b[3];
    double distance;
    double axis_a[3], axis_b[3]; // XPBD_JOINT_HINGE
    uint32_t kind, reserved;
};

// xpbd_joint_limit, device copy.
struct JointLimit {
    uint32_t joint, kind;
    double ref_a[3], ref_b[3]; // XPBD_LIMIT_HINGE / _TWIST
    double lower, upper;
};

// One extra term of a joint (k_joint_extras): an xpbd_joint_drive as it is (kind = XPBD_DRIVE_*), or the joint's
// XPBD_LIMIT_SLIDE (kind = kExtraSlideLimit: target = lower, compliance = upper; refs and max_force unused).
struct JointExtraItem {
    uint32_t joint, kind;
    double ref_a[3], ref_b[3];
    double target, compliance, max_force;
};
constexpr uint32_t kExtraSlideLimit = 0x100u;
constexpr uint32_t kJointExtraDoubles = 8; // a joint end's summed extra entries: dpos[3], drot[4] (s, x, y, z), count

// The uniform grid of one broadphase (device, written by k_grid).
struct GridInfo {
    double edge;        // cell edge = 2 * largest bounding radius
    int32_t origin[3];  // dense mode: cell of the box's minimum corner, minus the margin cell
    uint32_t dims[3];   //             cells per axis including the margins
    uint32_t dense;     // 1: bucket key = linear cell index (no two cells share a bucket); 0: hashed cell
};

// Device buffers of the contact pipeline (owned by the world, sized by the host).
struct ContactBuffers {
    // broadphase, per body
    double *centers;        // [3][stride] bounding-sphere centre (frame * centroid)
    double *radius;         // [stride]    r_shape + min(|v| dt, r_shape) + pad
    int32_t *cell;          // [3][stride] grid cell of the centre
    uint32_t *key;          // [stride]    hash bucket of that cell
    GridInfo *grid;         // [1]
    double *grid_partials;  // [workgroups of k_bounds][7] largest radius, min xyz, max xyz of the centres
    // hash table, table_size = power of two
    uint32_t *bucket_start; // [table_size + 1] counts -> exclusive scan
    uint32_t *bucket_cursor;// [table_size]
    uint32_t *items;        // [n] body ids grouped by bucket, ascending inside a bucket
    uint32_t *items_unsorted; // [n] the same in scatter (arrival) order
    uint32_t table_size;
    double *slot_sphere;    // [4][stride] centre xyz and radius of items[s], i.e. in bucket order
    int32_t *slot_cell;     // [3][stride] cell of items[s]
    // neighbour lists (CSR, ascending) and the pair list i < j
    uint32_t *nbr_off;      // [n + 1]
    uint32_t *pair_first;   // [n + 1]
    uint32_t *upper_start;  // [n]  index in nbr of b's first neighbour > b
    uint32_t *nbr;          // [entries]
    uint32_t *nbr_pair;     // [entries] pair index of (min, max)
    uint32_t *pairs;        // [n_pairs][2]
    // per substep
    double *rec;            // [stride][kRecDoubles] BodyRecord of this substep (xpbd_device.hpp): frames before / after
                            //   integrate, pose after the ground contacts, position before integrate
    const double *stat_rec; // [stride][kStatRecDoubles] StatRecord: inverse mass, inverse inertia, centre of mass
    const uint32_t *stat_index; // NULL: stat_rec is indexed by body; else stat_rec[stat_index[body]] (mass properties shared per shape)
    ContactManifold *manifolds; // [n_pairs]
    uint8_t *pair_codes;    // [n_pairs] n_points | feature << 4 of every pair (xpbd_pairs.h)
    unsigned long long *stats; // [2] touching pairs, manifold points (summed over substeps)
    uint32_t *scan_scratch; // block totals of the scans
    // joints: CSR body -> incident joints (ascending joint index); joint_off is NULL when there are none
    const Joint *joints;
    const uint32_t *joint_off;   // [n + 1]
    const uint32_t *joint_list;  // [2 * n_joints]
    // joint limits: CSR joint -> its limits (the caller's order); limit_off is NULL when there are none
    const JointLimit *limits;
    const uint32_t *limit_off;   // [n_joints + 1]
    double max_depenetration_speed; // 0 = off: xpbd_world_set_max_depenetration_speed
    // collision filters (xpbd_world_set_collision_filters): NULL = none, every pair may touch.  (Last: the kernel arguments
    // before them keep their offsets, so the kernels of a world without filters load exactly what they loaded before.)
    const uint2 *filter;    // [n] group, mask of every body
    uint32_t *slot_filter;  // [2][stride] group, mask of items[s] (bucket order; written only when `filter` is set)
    uint32_t filter_jointed; // XPBD_FILTER_JOINTED: bodies joined by a joint of `joints` are never neighbours
    // contact materials (xpbd_world_set_materials): NULL = off, every contact is the reference's (the kernels' plain forms,
    // which never read these two).  (After the filters, for the same reason.)
    const double *friction;  // [n] Coulomb coefficient of every body, >= 0, may be +inf
    double ground_friction;  // ... and of the plane z = 0
    // restitution (xpbd_world_set_restitution): NULL = off, no velocity pass is launched.  (Last again.)
    const double *restitution; // [n] coefficient of every body, in [0, 1]
    double ground_restitution; // ... and of the plane z = 0
    double bounce_threshold;   // a contact bounces only when it closed faster than this at the start of the substep
    // sliders and joint drives (xpbd.h, XPBD_JOINT_SLIDER / XPBD_LIMIT_SLIDE / xpbd_joint_drive): NULL = none, no kernel of
    // their own is launched and the pair solve loads nothing.  (Last again.)  k_joint_extras evaluates the extra entries of
    // the joints extra_joints[0..n_extra_joints) once per substep and leaves their sums for the pair solve to add.
    double *joint_extra;               // [2 * n_joints][kJointExtraDoubles] one record per entry of joint_list: the sum for that body
                                       //   and joint; zero for a joint without extras.  (Indexed by the slot a body's loop is at
                                       //   anyway: indexed by 2 * joint + end the 8-lane pair solve took two more VGPRs)
    const uint32_t *extra_joints;      // [n_extra_joints] the joints with extras, ascending
    const uint32_t *extra_slots;       // [2 * n_extra_joints] where in joint_list end a / end b of extra_joints[t] sits
    const uint32_t *extra_off;         // [n_extra_joints + 1] CSR into extra_items: the SLIDE limit first, then the drives in the caller's order
    const JointExtraItem *extra_items;
    uint32_t n_extra_joints;
    // heightfield terrain (xpbd_world_set_terrain): planes == NULL = none, the ground is the plane z = 0 and no kernel reads this.
    // (Last again.)  With one, the integrate + ground stage and the restitution pass run their TERRAIN forms; the fused
    // pair-solve + integrate + ground kernel has none, so the step runs the unfused schedule.
    Terrain terrain;
};

// Sleeping (xpbd_world_set_sleeping): which bodies are inert -- asleep or fixed -- as the frame started.  A pair whose two ends
// are both inert is no neighbour pair.  Default: none, the broadphase launches the kernels it launched before; with a table it
// launches the forms that take this as one more argument (ContactBuffers and the kernels that take it stay as they are).
struct InertBodies {
    const uint8_t *inert = nullptr; // [n]
    uint8_t *slot_inert = nullptr;  // [stride] inert[items[s]] (bucket order, written by launch_build_buckets)
};

// Which bodies a per-body kernel of the pipeline works on.  Default: all of them.  The multi-GPU world (xpbd_multi.cpp) runs
// the BOUNDARY bodies first, with their end-of-substep state exported straight into the halo send buffer, starts the
// exchange, runs the interior bodies meanwhile (`skip` marks boundary and ghost bodies), and finally gives the ghosts their
// owners' state from the gathered buffer.
struct BodySubset {
    const uint32_t *list = nullptr;        // NULL: bodies 0..n (minus `skip`); else the bodies list[0..count)
    uint32_t count = 0;
    const uint8_t *skip = nullptr;         // with list == NULL: bodies with skip[i] != 0 are left out
    double *export_rows = nullptr;         // with list (pair-solve kernels): the end-of-substep state of list[k] -> row k (13 doubles)
    const double *import_buf = nullptr;    // with list (integrate kernel): the state of list[k] comes from row import_rows[k]
    const uint32_t *import_rows = nullptr;
};

// ---- broadphase (once per step call) -------------------------------------------------------------
hipError_t launch_bounds_and_cells(const BodyArrays &b, const PolytopeTables &t, const double *shape_radius,
                                   double dt, double pad, const ContactBuffers &c, hipStream_t stream);
hipError_t launch_build_buckets(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert = InertBodies());
// counts into nbr_off / pair_first (then scanned in place; totals at [n])
hipError_t launch_neighbour_count(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert = InertBodies());
hipError_t launch_neighbour_fill(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert = InertBodies());

// ---- per substep -----------------------------------------------------------------------------------
// integrate + ground contacts (sequential per body): reads b.dyn, writes the body's record (frames, pose') into c.rec
hipError_t launch_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                   uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row, hipStream_t stream,
                                   const BodySubset &subset = BodySubset());
// SAT of every neighbour pair on the post-integrate frames
// (list: NULL = pre-test inside the SAT kernel, else the two-pass form of launch_sat_pairs; dense: many of the pairs touch)
hipError_t launch_sat_contact_pairs(const BodyArrays &b, const PolytopeTables &t, const ContactBuffers &c,
                                    uint32_t n_pairs, SatScratch *list, hipStream_t stream, bool dense = false);
// Jacobi pair solve + derive: reads the records, writes all 13 dynamic fields to dyn_out (b.dyn itself is fine: nobody
// reads another body's SoA state here)
hipError_t launch_pair_solve_derive(const BodyArrays &b, double *dyn_out, double h, const ContactBuffers &c,
                                    hipStream_t stream, const BodySubset &subset = BodySubset());

// launch_pair_solve_derive of this substep and launch_integrate_ground of the next one in a single kernel: the next
// substep's records go to next_rec (a second set: the records in `c` are still being read by the other bodies); the SoA
// state is NOT written (the records carry everything from substep to substep; the step's last launch_pair_solve_derive
// writes it).
hipError_t launch_pair_solve_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                              double *next_rec, uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row,
                                              hipStream_t stream, const BodySubset &subset = BodySubset());

// Sliders and joint drives (only when c.joint_extra is set): the extra entries of every listed joint from the records of this
// substep, summed per joint end into c.joint_extra, which the pair-solve kernels of the same substep add.
hipError_t launch_joint_extras(double h, const ContactBuffers &c, hipStream_t stream);

// Restitution, the velocity pass after derive (only when c.restitution is set): `post` holds the 13 dynamic fields after derive
// (the dyn_out of launch_pair_solve_derive; NOT b.dyn), `start` velocity and angular velocity at the start of the substep
// ([6][stride]: fields D_VEL.. of b.dyn before launch_integrate_ground), ground_masks the masks of launch_integrate_ground.
// Every body's end-of-substep state (pose copied, velocities updated) goes to b.dyn, which no lane of the launch reads.
// With subset.skip (the sleepers of a world with sleeping on) the bodies it marks end as `post` holds them: the caller has put
// their state there, the pass runs over everybody and they are put back from it.  (No list form.)
hipError_t launch_restitution(const BodyArrays &b, const double *post, const double *start, const ShapeTable &s, const ContactBuffers &c,
                              const uint32_t *ground_masks, hipStream_t stream, const BodySubset &subset = BodySubset());

// Heightfield terrain.  The plane table of a field from its heights (device, ny rows of nx): both triangles of every cell into
// planes[cell][8], `t` describing the field (t.planes is not read).  And the terrain at n points xy[2k..] (device arrays):
// height[k] and, unless normal_xyz is NULL, the unit normal; NaN and (0, 0, 0) outside the field.
hipError_t launch_terrain_planes(const double *heights, const Terrain &t, double *planes, hipStream_t stream);
hipError_t launch_sample_terrain(const Terrain &t, const double *xy, uint32_t n, double *height, double *normal_xyz, hipStream_t stream);

// Rigid::frame() of all bodies from the SoA state into the post-integrate frame of their records (all the diagnostic
// narrowphase entry points need); and the StatRecords from the SoA static fields (after an upload).
hipError_t launch_body_frames(const BodyArrays &b, double *rec, hipStream_t stream);
hipError_t launch_stat_records(const BodyArrays &b, double *stat_rec, hipStream_t stream);
// ... and body-major, frames[7 * i + f], for the host read-back.
hipError_t launch_body_frames_aos(const BodyArrays &b, double *frames, hipStream_t stream);

// The exclusive scan the broadphase uses is a unit of its own (xpbd_scan.h), and so are the per-body utilities that are no
// contact code -- halo export / import, body edits, halo validity, the re-plan kernels (xpbd_body_ops.h).

} // namespace xpbd
