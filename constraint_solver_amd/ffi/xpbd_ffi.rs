//! xpbd_ffi.rs -- Rust binding of include/xpbd.h for jim-ec/constraint_solver.
//!
//! NOT COMPILED IN THIS REPOSITORY: the build image has no rustc/cargo.  This is the
//! binding a maintainer of the reference adds (as `src/xpbd_ffi.rs`, plus
//! `println!("cargo:rustc-link-lib=dylib=xpbd_hip")` in build.rs) to run the per-substep
//! hot path on an MI355X.  The compiled and tested equivalent in this repository is the C++
//! host mirror `constraint_solver_amd/host/constraint_solver.hpp`, which calls the very same
//! extern "C" entry points.
//!
//! What it replaces in the reference:
//!   solver::step        src/solver.rs:3-17   -> xpbd_step_one      (literal, one body)
//!   World::integrate    src/world.rs:34-43   -> xpbd_world_step    (batched, state stays in HBM)
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

use cgmath::{Matrix3, Quaternion, Vector3};

use crate::{geometry::Polytope, rigid::Rigid};

/// repr(C) mirror of `Rigid` (src/rigid.rs:6-50), `color` dropped: 38 f64.
/// cgmath's own structs are not repr(C)-stable (Quaternion stores v before s in 0.18),
/// so the conversion is spelled out field by field.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdRigid {
    pub inverse_mass: f64,
    pub inverse_inertia: [f64; 9], // column-major, [3 * col + row]
    pub external_force: [f64; 3],
    pub internal_force: [f64; 3],
    pub external_torque: [f64; 3],
    pub internal_torque: [f64; 3],
    pub velocity: [f64; 3],
    pub angular_velocity: [f64; 3],
    pub center_of_mass: [f64; 3],
    pub position: [f64; 3],
    pub rotation: [f64; 4], // s, x, y, z  (Quaternion::new argument order)
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdContact {
    pub body: u32,
    pub vertex: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdConfig {
    pub struct_size: u32,
    pub device: i32,
    pub mode: u32,
    pub flags: u32,
    pub block_size: u32,
    pub reserved: [u32; 3],
}

/// EXTENSION (not in the reference): full polytope topology for body-body contacts.
#[repr(C)]
pub struct XpbdPolytope {
    pub vertices_xyz: *const f64,
    pub edges: *const u32,
    pub face_offsets: *const u32,
    pub face_indices: *const u32,
    pub n_vertices: u32,
    pub n_edges: u32,
    pub n_faces: u32,
    pub reserved: u32,
    pub centroid: [f64; 3],
}

/// EXTENSION: contact manifold of one body pair.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct XpbdManifold {
    pub n_points: u32,
    pub feature: u32,
    pub index_a: u32,
    pub index_b: u32,
    pub separation: f64,
    pub p_ref: [[f64; 3]; 8],
    pub p_inc: [[f64; 3]; 8],
}

/// EXTENSION: distance / ball joint between two bodies (a hinge is two ball joints on its axis).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdJoint {
    pub body_a: u32,
    pub body_b: u32,
    pub anchor_a: [f64; 3],
    pub anchor_b: [f64; 3],
    pub distance: f64,
    pub axis_a: [f64; 3], // XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER: unit axes in the object space of a / b that the joint keeps aligned
    pub axis_b: [f64; 3],
    pub kind: u32,        // XPBD_JOINT_DISTANCE = 0, XPBD_JOINT_HINGE = 1, XPBD_JOINT_SLIDER = 2
    pub reserved: u32,
}

/// EXTENSION: one entry of the kinematic table (xpbd_kinematic, 64 bytes; see xpbd.h, "KINEMATIC bodies"): a fixed body that
/// moves on a script.
pub const XPBD_KINEMATIC_POSE: u32 = 0;     // linear = target position, angular = target rotation {s, x, y, z}
pub const XPBD_KINEMATIC_VELOCITY: u32 = 1; // linear = velocity, angular = {wx, wy, wz, ignored}
pub const XPBD_MASS_INVERSE: u32 = 0; // row = inverse_mass, inverse_inertia[9], center_of_mass[3]
pub const XPBD_MASS_DIRECT: u32 = 1; // row = mass, inertia[9], center_of_mass[3]: inverted on the device
pub const XPBD_MASS_KEEP_FRAME: u32 = 0x100; // the geometry stays where it is when center_of_mass changes
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdKinematic {
    pub body: u32,
    pub mode: u32,
    pub linear: [f64; 3],
    pub angular: [f64; 4],
}

/// EXTENSION: damping row of a body and damper of a joint (see xpbd.h, "DAMPING").  The default row is
/// {0.0, 0.0, f64::INFINITY, f64::INFINITY}.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct XpbdBodyDamping {
    pub linear: f64,
    pub angular: f64,
    pub max_linear_speed: f64,
    pub max_angular_speed: f64,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdJointDamping {
    pub joint: u32,
    pub reserved: u32, // must be 0
    pub linear: f64,
    pub angular: f64,
}

/// EXTENSION: drive of a joint (XPBD_DRIVE_ANGLE = 0, XPBD_DRIVE_ANGULAR_VELOCITY = 1, XPBD_DRIVE_POSITION = 2,
/// XPBD_DRIVE_VELOCITY = 3; see xpbd.h, "SLIDERS and joint DRIVES").
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdJointDrive {
    pub joint: u32,       // index into the joints of the last xpbd_world_set_joints
    pub kind: u32,
    pub ref_a: [f64; 3],  // angular kinds: unit vectors perpendicular to axis_a / axis_b, object space of a / b
    pub ref_b: [f64; 3],
    pub target: f64,      // rad, rad/s, m, m/s
    pub compliance: f64,  // >= 0, finite
    pub max_force: f64,   // > 0, +inf allowed
}

/// EXTENSION: xpbd_joint_state (80 bytes): what xpbd_world_joint_states reports of one joint (see xpbd.h, "Joint STATES and
/// drive TARGETS"); a field whose XPBD_JOINT_STATE_HAS_* flag is clear is +0.0.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdJointState {
    pub separation: f64,   // DISTANCE, HINGE: |d| - distance; SLIDER: |d - a_w s|
    pub misalignment: f64, // HINGE, SLIDER: |a_w x b_w|
    pub angle: f64,        // rad, in [-pi, pi]
    pub angle_rate: f64,   // rad/s
    pub travel: f64,       // SLIDER: m
    pub travel_rate: f64,  // m/s
    pub swing: f64,        // DISTANCE with a SWING or TWIST limit: rad
    pub twist: f64,        // DISTANCE with a TWIST limit: rad
    pub joint: u32,
    pub kind: u32,         // XPBD_JOINT_*; XPBD_JOINT_STATE_NO_JOINT: the index was out of range (device variant)
    pub flags: u32,        // XPBD_JOINT_STATE_*
    pub reserved: u32,
}
pub const XPBD_JOINT_STATE_HAS_ANGLE: u32 = 0x001;
pub const XPBD_JOINT_STATE_HAS_TRAVEL: u32 = 0x002;
pub const XPBD_JOINT_STATE_HAS_SWING: u32 = 0x004;
pub const XPBD_JOINT_STATE_HAS_TWIST: u32 = 0x008;
pub const XPBD_JOINT_STATE_ANGLE_OF_DRIVE: u32 = 0x010;
pub const XPBD_JOINT_STATE_ANGLE_BELOW: u32 = 0x100;
pub const XPBD_JOINT_STATE_ANGLE_ABOVE: u32 = 0x200;
pub const XPBD_JOINT_STATE_TRAVEL_BELOW: u32 = 0x400;
pub const XPBD_JOINT_STATE_TRAVEL_ABOVE: u32 = 0x800;
pub const XPBD_JOINT_STATE_SWING_ABOVE: u32 = 0x1000;
pub const XPBD_JOINT_STATE_TWIST_BELOW: u32 = 0x2000;
pub const XPBD_JOINT_STATE_TWIST_ABOVE: u32 = 0x4000;
pub const XPBD_JOINT_STATE_NO_JOINT: u32 = 0xFFFF_FFFF;

/// EXTENSION: limit of a joint (XPBD_LIMIT_HINGE = 0, XPBD_LIMIT_SWING = 1, XPBD_LIMIT_TWIST = 2: angular, radians;
/// XPBD_LIMIT_SLIDE = 3: the travel of a slider, metres; see xpbd.h).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdJointLimit {
    pub joint: u32,       // index into the joints of the last xpbd_world_set_joints
    pub kind: u32,
    pub ref_a: [f64; 3],  // HINGE, TWIST: unit vectors perpendicular to axis_a / axis_b, object space of a / b
    pub ref_b: [f64; 3],
    pub lower: f64,       // radians, -pi <= lower <= upper <= pi (SWING: lower = 0)
    pub upper: f64,
}

/// EXTENSION: collision filter of one body: bodies i, j may touch iff group_i & mask_j != 0 && group_j & mask_i != 0.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct XpbdCollisionFilter {
    pub group: u32, // the layers this body is in
    pub mask: u32,  // the layers it collides with
}

impl Default for XpbdCollisionFilter {
    fn default() -> Self {
        XpbdCollisionFilter { group: !0u32, mask: !0u32 }
    }
}

pub const XPBD_FILTER_JOINTED: u32 = 1;

/// EXTENSION: contact material of one body: Coulomb friction at the position level (a contact uses the smaller coefficient
/// of its two sides; +inf, the default, is the reference's contact).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct XpbdMaterial {
    pub friction: f64, // >= 0, may be +inf
    pub reserved: f64, // must be 0 (room for restitution)
}

impl Default for XpbdMaterial {
    fn default() -> Self {
        XpbdMaterial { friction: f64::INFINITY, reserved: 0.0 }
    }
}

/// EXTENSION: heightfield terrain, the ground of XPBD_MODE_CONTACTS in place of the plane z = 0 (xpbd_world_set_terrain); 48 bytes.
pub const XPBD_MAX_TERRAIN_SAMPLES: u32 = 1 << 22;
#[repr(C)]
#[derive(Clone, Copy)]
pub struct XpbdHeightfield {
    pub nx: u32,               // samples along x and y, each >= 2, nx * ny <= XPBD_MAX_TERRAIN_SAMPLES
    pub ny: u32,
    pub origin: [f64; 2],      // world x, y of sample (0, 0)
    pub cell: [f64; 2],        // spacing along x and y: finite, > 0
    pub heights: *const f64,   // ny rows of nx: heights[iy * nx + ix], all finite; copied
}

/// EXTENSION: body edits -- one impulse on a resident body (xpbd_world_apply_impulses); 80 bytes.
pub const XPBD_IMPULSE_AT_POINT: u32 = 0; // the impulse acts at `point` (world space)
pub const XPBD_IMPULSE_AT_CENTRE: u32 = 1; // ... at position + center_of_mass; `point` is ignored
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdImpulse {
    pub body: u32,
    pub flags: u32,                // XPBD_IMPULSE_*
    pub impulse: [f64; 3],         // N s, world space
    pub point: [f64; 3],           // world space
    pub angular_impulse: [f64; 3], // N m s, world space
}

/// EXTENSION: result of the GJK + EPA narrowphase for one pair.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct XpbdGjkResult {
    pub status: i32,
    pub gjk_iterations: u32,
    pub epa_iterations: u32,
    pub reserved: u32,
    pub depth: f64,
    pub normal: [f64; 3],
    pub point_a: [f64; 3],
    pub point_b: [f64; 3],
}

/// xpbd_edge_query: the reference's edge_axes_separation result, (f64::MIN, (usize::MAX, usize::MAX)) as (-DBL_MAX, !0, !0)
#[repr(C)]
pub struct XpbdEdgeQuery {
    pub separation: f64,
    pub edge_a: u32,
    pub edge_b: u32,
}

pub const XPBD_NO_HIT: u32 = 0xFFFF_FFFF;
pub const XPBD_RAY_INSIDE: u32 = 0xFFFF_FFFF;
pub const XPBD_RAYCAST_BRUTE_FORCE: u32 = 1;
/// EXTENSION: a flag of the raycast, overlap and sweep calls of xpbd_world alike: the heightfield of xpbd_world_set_terrain answers
/// too (XPBD_E_INVALID without one; an unknown flag for xpbd_multi_world_*).  A hit on it has body = XPBD_HIT_TERRAIN and face = the
/// triangle 2 * (j * (nx - 1) + i) + k (XPBD_RAY_INSIDE from in or under the ground); an overlap's entry for it is the last of its segment.
pub const XPBD_QUERY_TERRAIN: u32 = 0x100;
pub const XPBD_HIT_TERRAIN: u32 = 0xFFFF_FFFE;

/// xpbd_ray (64 bytes): distances are in units of |direction|; ignore_body = XPBD_NO_HIT for none; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdRay {
    pub origin: [f64; 3],
    pub direction: [f64; 3],
    pub max_distance: f64,
    pub ignore_body: u32,
    pub reserved: u32,
}

/// xpbd_ray_hit (64 bytes): body = XPBD_NO_HIT on a miss; face = XPBD_RAY_INSIDE when the ray starts inside the body
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdRayHit {
    pub body: u32,
    pub face: u32,
    pub distance: f64,
    pub point: [f64; 3],
    pub normal: [f64; 3],
}

pub const XPBD_OVERLAP_BRUTE_FORCE: u32 = 1;
pub const XPBD_OVERLAP_MASKED: u32 = 2;

pub const XPBD_SWEEP_INITIAL: u32 = 3;
pub const XPBD_SWEEP_BRUTE_FORCE: u32 = 1;
pub const XPBD_SWEEP_MASKED: u32 = 2;
pub const XPBD_SWEEP_BRUTE_FORCE_SWEEPS: u32 = 8;

/// xpbd_sweep (104 bytes): the convex volume `shape` at the frame {position, rotation {s, x, y, z}}, moved by t * direction for t in
/// [0, max_distance]; ignore_body = XPBD_NO_HIT for none; mask is read with XPBD_SWEEP_MASKED only; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdSweep {
    pub position: [f64; 3],
    pub rotation: [f64; 4],
    pub direction: [f64; 3],
    pub max_distance: f64,
    pub shape: u32,
    pub ignore_body: u32,
    pub mask: u32,
    pub reserved: u32,
}

/// xpbd_sweep_hit (72 bytes): the first body the volume hits (XPBD_NO_HIT: none) at t = distance; feature = XPBD_FEATURE_* (A = the
/// volume, B = the body) or XPBD_SWEEP_INITIAL; position = the volume's frame position at the impact; normal out of the body
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdSweepHit {
    pub body: u32,
    pub feature: u32,
    pub face: u32,
    pub reserved: u32,
    pub distance: f64,
    pub position: [f64; 3],
    pub normal: [f64; 3],
}

pub const XPBD_DISTANCE_BRUTE_FORCE: u32 = 1;
pub const XPBD_DISTANCE_MASKED: u32 = 2;
pub const XPBD_DISTANCE_OVERLAP: u32 = 3;
pub const XPBD_DISTANCE_POINT: u32 = 0xFFFF_FFFF;
pub const XPBD_DISTANCE_BRUTE_FORCE_QUERIES: u32 = 8;

/// xpbd_distance_query (80 bytes): the convex volume `shape` at the frame {position, rotation {s, x, y, z}}, or the point `position`
/// with shape = XPBD_DISTANCE_POINT; bodies further than max_distance do not answer; ignore_body = XPBD_NO_HIT for none; mask is
/// read with XPBD_DISTANCE_MASKED only; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdDistanceQuery {
    pub position: [f64; 3],
    pub rotation: [f64; 4],
    pub max_distance: f64,
    pub shape: u32,
    pub ignore_body: u32,
    pub mask: u32,
    pub reserved: u32,
}

/// xpbd_distance_hit (96 bytes): the nearest body (XPBD_NO_HIT: none within max_distance); feature = XPBD_FEATURE_* (A = the volume,
/// B = the body) with the indices of the two closest features, or XPBD_DISTANCE_OVERLAP at distance 0; the closest points in
/// world space; normal from the body to the volume
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdDistanceHit {
    pub body: u32,
    pub feature: u32,
    pub index_a: u32,
    pub index_b: u32,
    pub distance: f64,
    pub point_a: [f64; 3],
    pub point_b: [f64; 3],
    pub normal: [f64; 3],
}

/// xpbd_overlap_query (72 bytes): a convex volume, shape `shape` of the polytope table at the frame {position, rotation {s, x, y, z}};
/// ignore_body = XPBD_NO_HIT for none; mask is read with XPBD_OVERLAP_MASKED only; reserved = 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdOverlapQuery {
    pub position: [f64; 3],
    pub rotation: [f64; 4],
    pub shape: u32,
    pub ignore_body: u32,
    pub mask: u32,
    pub reserved: u32,
}

/// EXTENSION: xpbd_sensor_hit (8 bytes; see xpbd.h, "SENSOR bodies"): a body that touched a sensor in the report frame, and the
/// index of the pair's record in xpbd_world_download_pair_contacts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct XpbdSensorHit {
    pub body: u32,
    pub pair: u32,
}

/// xpbd_overlap_hit (16 bytes): a body the volume touches; feature = XPBD_FEATURE_* (A = the volume, B = the body), separation < 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdOverlapHit {
    pub body: u32,
    pub feature: u32,
    pub separation: f64,
}

pub const XPBD_CONTACT_BEGIN: u32 = 0;
pub const XPBD_CONTACT_END: u32 = 1;

/// xpbd_pair_contact (64 bytes): a pair that touched in the frame; manifold of its last substep (include/xpbd.h, "Contact REPORTS")
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdPairContact {
    pub body_a: u32,
    pub body_b: u32,
    pub substeps: u32,
    pub n_points: u32,
    pub feature: u32,
    pub first_point: u32,
    pub reserved: [u32; 2],
    pub normal: [f64; 3],
    pub depth: f64,
}

/// xpbd_contact_point (48 bytes, world space)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdContactPoint {
    pub p_ref: [f64; 3],
    pub p_inc: [f64; 3],
}

/// xpbd_contact_event (12 bytes): kind = XPBD_CONTACT_BEGIN / XPBD_CONTACT_END
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdContactEvent {
    pub body_a: u32,
    pub body_b: u32,
    pub kind: u32,
}

pub const XPBD_ISLAND_NONE: u32 = 0xFFFF_FFFF;
pub const XPBD_ISLANDS_NO_JOINTS: u32 = 1;
pub const XPBD_ISLANDS_NO_CONTACTS: u32 = 2;

/// xpbd_island (40 bytes): one connected group of non-fixed bodies (include/xpbd.h, "Contact ISLANDS")
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdIsland {
    pub first_body: u32,
    pub n_bodies: u32,
    pub n_pairs: u32,
    pub n_joints: u32,
    pub n_anchors: u32,
    pub n_grounded: u32,
    pub max_speed2: f64,
    pub max_angular_speed2: f64,
}

pub const XPBD_SLEEP_GROUP_NONE: u32 = 0xFFFF_FFFF;

/// xpbd_sleep_config (24 bytes): the thresholds of island sleeping (include/xpbd.h, "SLEEPING")
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct XpbdSleepConfig {
    pub linear_speed: f64,
    pub angular_speed: f64,
    pub frames_to_sleep: u32,
    pub flags: u32,
}

#[repr(C)]
pub struct XpbdWorld {
    _private: [u8; 0],
}

#[repr(C)]
pub struct XpbdMultiWorld {
    _private: [u8; 0],
}

pub const XPBD_COMM_ID_BYTES: usize = 128;
pub const XPBD_TRANSPORT_RCCL: u32 = 0;
pub const XPBD_TRANSPORT_LOCAL: u32 = 1;
pub const XPBD_MULTI_AUTO_REPLAN: u32 = 1;
pub const XPBD_MULTI_PLAN_THROUGH_DEVICE: u32 = 2;
pub const XPBD_E_HALO: c_int = -7;

/// xpbd_multi_config (include/xpbd.h)
#[repr(C)]
pub struct XpbdMultiConfig {
    pub struct_size: u32,
    pub n_ranks: u32,
    pub first_rank: u32,
    pub n_local: u32,
    pub devices: *const i32,
    pub transport: u32,
    pub flags: u32,
    pub comm_id: *const u8,
    pub contact_pad: f64,
    pub halo_margin: f64,
    pub narrowphase: u32,
    pub reserved: u32,
}

#[link(name = "xpbd_hip")]
extern "C" {
    pub fn xpbd_abi_version() -> u32;
    pub fn xpbd_last_error() -> *const c_char;
    pub fn xpbd_config_default(cfg: *mut XpbdConfig);
    pub fn xpbd_device_count() -> c_int;
    pub fn xpbd_world_create(out: *mut *mut XpbdWorld, cfg: *const XpbdConfig) -> c_int;
    pub fn xpbd_world_destroy(w: *mut XpbdWorld);
    pub fn xpbd_world_set_shapes(w: *mut XpbdWorld, verts_xyz: *const f64, vert_offsets: *const u32, n_shapes: u32) -> c_int;
    pub fn xpbd_world_upload_bodies(w: *mut XpbdWorld, aos: *const XpbdRigid, shape_id: *const u32, n: u32) -> c_int;
    pub fn xpbd_world_download_bodies(w: *mut XpbdWorld, aos: *mut XpbdRigid, n: u32) -> c_int;
    pub fn xpbd_world_body_count(w: *const XpbdWorld) -> u32;
    pub fn xpbd_world_step(w: *mut XpbdWorld, dt: f64, substeps: u32) -> c_int;
    pub fn xpbd_world_synchronize(w: *mut XpbdWorld) -> c_int;
    pub fn xpbd_world_download_contacts(w: *mut XpbdWorld, out: *mut XpbdContact, cap: u32, n_out: *mut u32) -> c_int;
    pub fn xpbd_world_download_contact_masks(w: *mut XpbdWorld, masks: *mut u32, substeps: u32, n: u32) -> c_int;
    pub fn xpbd_world_set_stream(w: *mut XpbdWorld, hip_stream: *mut c_void) -> c_int;
    pub fn xpbd_world_get_stream(w: *const XpbdWorld) -> *mut c_void;
    pub fn xpbd_world_set_mode(w: *mut XpbdWorld, mode: u32) -> c_int;
    pub fn xpbd_step_one(rigid: *mut XpbdRigid, verts_xyz: *const f64, nverts: u32, dt: f64, substeps: u32) -> c_int;
    pub fn xpbd_selftest_div_sqrt(device: i32, a: *const f64, b: *const f64, q: *mut f64, r: *mut f64, n: u32) -> c_int;
    pub fn xpbd_selftest_exact_math(device: i32, x: *const f64, a: *const f64, h: f64, n: u32, fast: *mut f64, plain: *mut f64) -> c_int;
    pub fn xpbd_selftest_hbm_copy(device: i32, bytes: u64, repeats: u32, gbytes_per_s: *mut f64) -> c_int;
    pub fn xpbd_selftest_field_streams(device: i32, bodies: u64, tile_major: u32, repeats: u32, gbytes_per_s: *mut f64) -> c_int;
    pub fn xpbd_selftest_gather(device: i32, records: u32, record_bytes: u32, read_bytes: u32, repeats: u32, gbytes_per_s: *mut f64) -> c_int;
    pub fn xpbd_world_download_frames(w: *mut XpbdWorld, frames: *mut f64, n: u32) -> c_int;
    // ---- extension: body-body contacts, joints, multi-GPU halo exchange (not in the reference) ----
    pub fn xpbd_world_set_polytopes(w: *mut XpbdWorld, shapes: *const XpbdPolytope, n_shapes: u32) -> c_int;
    pub fn xpbd_world_narrowphase(w: *mut XpbdWorld, pairs: *const u32, n_pairs: u32, out: *mut XpbdManifold) -> c_int;
    pub fn xpbd_world_edge_axes_separation(w: *mut XpbdWorld, pairs: *const u32, n_pairs: u32, out: *mut XpbdEdgeQuery) -> c_int;
    pub fn xpbd_world_narrowphase_gjk(w: *mut XpbdWorld, pairs: *const u32, n_pairs: u32, out: *mut XpbdGjkResult) -> c_int;
    pub fn xpbd_world_set_narrowphase(w: *mut XpbdWorld, narrowphase: u32) -> c_int;
    pub fn xpbd_world_set_sat_schedule(w: *mut XpbdWorld, schedule: u32) -> c_int;
    pub fn xpbd_world_set_contact_pad(w: *mut XpbdWorld, pad: f64) -> c_int;
    pub fn xpbd_world_contact_stats(w: *mut XpbdWorld, out: *mut u64) -> c_int;
    pub fn xpbd_world_build_neighbours(w: *mut XpbdWorld, dt: f64, n_entries_out: *mut u32) -> c_int;
    pub fn xpbd_world_download_neighbours(w: *mut XpbdWorld, offsets: *mut u32, neighbours: *mut u32, cap: u32) -> c_int;
    pub fn xpbd_world_set_joints(w: *mut XpbdWorld, joints: *const XpbdJoint, n_joints: u32) -> c_int;
    pub fn xpbd_world_set_joint_limits(w: *mut XpbdWorld, limits: *const XpbdJointLimit, n_limits: u32) -> c_int;
    pub fn xpbd_world_set_joint_drives(w: *mut XpbdWorld, drives: *const XpbdJointDrive, n_drives: u32) -> c_int;
    pub fn xpbd_world_set_max_depenetration_speed(w: *mut XpbdWorld, speed: f64) -> c_int;
    pub fn xpbd_multi_world_set_max_depenetration_speed(mw: *mut XpbdMultiWorld, speed: f64) -> c_int;
    pub fn xpbd_world_snapshot_positions(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_snapshot: *mut f64) -> c_int;
    pub fn xpbd_world_max_displacement2(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_snapshot: *const f64, dev_scale: *const f64, dev_max: *mut f64) -> c_int;
    // ---- extension: the multi-GPU world (one call per frame; the library owns streams, RCCL communicators and the halo plan) ----
    pub fn xpbd_comm_unique_id(id: *mut u8) -> c_int;
    pub fn xpbd_comm_library() -> *const c_char;
    pub fn xpbd_multi_config_default(cfg: *mut XpbdMultiConfig);
    pub fn xpbd_multi_world_create(out: *mut *mut XpbdMultiWorld, cfg: *const XpbdMultiConfig) -> c_int;
    pub fn xpbd_multi_world_destroy(mw: *mut XpbdMultiWorld);
    pub fn xpbd_multi_world_set_polytopes(mw: *mut XpbdMultiWorld, shapes: *const XpbdPolytope, n_shapes: u32) -> c_int;
    pub fn xpbd_multi_world_upload(mw: *mut XpbdMultiWorld, bodies: *const XpbdRigid, shape_id: *const u32, first_global: u32, n_bodies: u32,
                                   n_global: u32, joints: *const XpbdJoint, n_joints: u32) -> c_int;
    pub fn xpbd_multi_world_set_joint_limits(mw: *mut XpbdMultiWorld, limits: *const XpbdJointLimit, n_limits: u32) -> c_int;
    pub fn xpbd_multi_world_set_joint_drives(mw: *mut XpbdMultiWorld, drives: *const XpbdJointDrive, n_drives: u32) -> c_int;
    pub fn xpbd_multi_world_step(mw: *mut XpbdMultiWorld, dt: f64, substeps: u32) -> c_int;
    pub fn xpbd_multi_world_replan(mw: *mut XpbdMultiWorld) -> c_int;
    pub fn xpbd_multi_world_synchronize(mw: *mut XpbdMultiWorld) -> c_int;
    pub fn xpbd_multi_world_download(mw: *mut XpbdMultiWorld, out: *mut XpbdRigid, n: u32) -> c_int;
    pub fn xpbd_multi_world_download_owned(mw: *mut XpbdMultiWorld, ids: *mut u32, out: *mut XpbdRigid, cap: u32, n_out: *mut u32) -> c_int;
    pub fn xpbd_multi_world_halo_stats(mw: *mut XpbdMultiWorld, out: *mut u64, max_displacement: *mut f64) -> c_int;
    pub fn xpbd_multi_world_plan_stats(mw: *mut XpbdMultiWorld, out: *mut u64) -> c_int; // out: [u64; 12]
    pub fn xpbd_multi_world_owners(mw: *mut XpbdMultiWorld, owner: *mut u8, n_global: u32) -> c_int;
    pub fn xpbd_multi_world_contact_stats(mw: *mut XpbdMultiWorld, out: *mut u64) -> c_int;
    pub fn xpbd_halo_cell_key(centre: *const f64, cell_edge: f64) -> i64;
    pub fn xpbd_halo_partition(cell_keys: *const i64, n_global: u32, n_ranks: u32, owner: *mut u8) -> c_int;
    pub fn xpbd_halo_plan_owned(cell_keys: *const i64, owner: *const u8, n_global: u32, n_ranks: u32, rank: u32, joints: *const XpbdJoint,
                                n_joints: u32, ghosts: *mut u32, n_ghosts: *mut u32, boundary: *mut u32, n_boundary: *mut u32, far: *mut u8,
                                cap: u32) -> c_int;
    pub fn xpbd_halo_plan_light(keys_at_cut: *const i64, cell_keys: *const i64, n_global: u32, n_ranks: u32, rank: u32, joints: *const XpbdJoint,
                                n_joints: u32, owner_now: *mut u8, own: *mut u32, n_own: *mut u32, ghosts: *mut u32, n_ghosts: *mut u32,
                                boundary: *mut u32, n_boundary: *mut u32, far: *mut u8, cap: u32) -> c_int;
    pub fn xpbd_halo_plan_far(cell_keys: *const i64, n_global: u32, n_ranks: u32, rank: u32, far: *mut u8, cap: u32, n_owned: *mut u32) -> c_int;
    pub fn xpbd_halo_plan(cell_keys: *const i64, n_global: u32, n_ranks: u32, rank: u32, joints: *const XpbdJoint, n_joints: u32,
                          ghosts: *mut u32, n_ghosts: *mut u32, boundary: *mut u32, n_boundary: *mut u32, cap: u32) -> c_int;
    pub fn xpbd_world_contacts_begin(w: *mut XpbdWorld, dt: f64) -> c_int;
    pub fn xpbd_world_contacts_substep(w: *mut XpbdWorld, h: f64) -> c_int;
    pub fn xpbd_world_export_dynamic(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_buf: *mut f64) -> c_int;
    pub fn xpbd_world_import_dynamic(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_buf: *const f64) -> c_int;
    pub fn xpbd_world_import_dynamic_rows(w: *mut XpbdWorld, dev_indices: *const u32, dev_rows: *const u32, n: u32, dev_buf: *const f64) -> c_int;
    // state history: replaces `states: Vec<(World, DebugLines)>` of src/app.rs:48 (see HistoryWorld below)
    pub fn xpbd_world_history_push(w: *mut XpbdWorld, index_out: *mut u32) -> c_int;
    pub fn xpbd_world_history_restore(w: *mut XpbdWorld, index: u32) -> c_int;
    pub fn xpbd_world_history_truncate(w: *mut XpbdWorld, length: u32) -> c_int;
    pub fn xpbd_world_history_length(w: *const XpbdWorld) -> u32;
    pub fn xpbd_world_raycast(w: *mut XpbdWorld, rays: *const XpbdRay, n_rays: u32, flags: u32, hits: *mut XpbdRayHit) -> c_int;
    pub fn xpbd_world_raycast_device(w: *mut XpbdWorld, dev_rays: *const XpbdRay, n_rays: u32, flags: u32, dev_hits: *mut XpbdRayHit)
        -> c_int;
    pub fn xpbd_multi_world_raycast(mw: *mut XpbdMultiWorld, rays: *const XpbdRay, n_rays: u32, flags: u32, hits: *mut XpbdRayHit)
        -> c_int;
    pub fn xpbd_world_set_collision_filters(w: *mut XpbdWorld, filters: *const XpbdCollisionFilter, n: u32, flags: u32) -> c_int;
    pub fn xpbd_multi_world_set_collision_filters(mw: *mut XpbdMultiWorld, filters: *const XpbdCollisionFilter, n_global: u32, flags: u32)
        -> c_int;
    pub fn xpbd_world_set_materials(w: *mut XpbdWorld, materials: *const XpbdMaterial, n: u32, ground_friction: f64) -> c_int;
    pub fn xpbd_multi_world_set_materials(mw: *mut XpbdMultiWorld, materials: *const XpbdMaterial, n_global: u32, ground_friction: f64)
        -> c_int;
    pub fn xpbd_world_set_restitution(w: *mut XpbdWorld, restitution: *const f64, n: u32, ground_restitution: f64, bounce_threshold: f64)
        -> c_int;
    // damping: rows NULL with n = 0 = the default row for every body; the joint list replaces the previous one (n = 0 clears)
    pub fn xpbd_world_set_damping(w: *mut XpbdWorld, rows: *const XpbdBodyDamping, n: u32) -> c_int;
    pub fn xpbd_world_get_damping(w: *mut XpbdWorld, rows: *mut XpbdBodyDamping, n: u32) -> c_int;
    pub fn xpbd_world_set_joint_damping(w: *mut XpbdWorld, list: *const XpbdJointDamping, n: u32) -> c_int;
    // terrain: hf NULL = back to the plane z = 0; sample_terrain takes host arrays and waits (normal_xyz may be NULL)
    pub fn xpbd_world_set_terrain(w: *mut XpbdWorld, hf: *const XpbdHeightfield) -> c_int;
    pub fn xpbd_world_sample_terrain(w: *mut XpbdWorld, xy: *const f64, n: u32, height: *mut f64, normal_xyz: *mut f64) -> c_int;
    // body edits: forces, impulses and state of resident bodies (host arrays wait; `_device`: device arrays, stream-ordered)
    pub fn xpbd_world_set_external_wrench(w: *mut XpbdWorld, indices: *const u32, n: u32, force_xyz: *const f64, torque_xyz: *const f64)
        -> c_int;
    pub fn xpbd_world_set_external_wrench_device(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_force_xyz: *const f64,
                                                 dev_torque_xyz: *const f64) -> c_int;
    pub fn xpbd_world_apply_impulses(w: *mut XpbdWorld, list: *const XpbdImpulse, n: u32) -> c_int;
    pub fn xpbd_world_apply_impulses_device(w: *mut XpbdWorld, dev_list: *const XpbdImpulse, n: u32) -> c_int;
    pub fn xpbd_world_set_dynamics(w: *mut XpbdWorld, indices: *const u32, n: u32, rows: *const f64) -> c_int;
    pub fn xpbd_world_get_dynamics(w: *mut XpbdWorld, indices: *const u32, n: u32, rows: *mut f64) -> c_int;
    pub fn xpbd_multi_world_set_external_wrench(mw: *mut XpbdMultiWorld, indices: *const u32, n: u32, force_xyz: *const f64,
                                                torque_xyz: *const f64) -> c_int;
    pub fn xpbd_multi_world_apply_impulses(mw: *mut XpbdMultiWorld, list: *const XpbdImpulse, n: u32) -> c_int;
    // Body POPULATION: removing resident bodies and appending new ones (include/xpbd.h); the maps use XPBD_NO_HIT for what is gone
    pub fn xpbd_world_remove_bodies(w: *mut XpbdWorld, indices: *const u32, n: u32, old_to_new: *mut u32, joint_old_to_new: *mut u32,
                                    n_bodies_out: *mut u32) -> c_int;
    pub fn xpbd_world_remove_bodies_device(w: *mut XpbdWorld, dev_remove: *const u8, dev_old_to_new: *mut u32, joint_old_to_new: *mut u32,
                                           n_bodies_out: *mut u32) -> c_int;
    pub fn xpbd_world_add_bodies(w: *mut XpbdWorld, aos: *const XpbdRigid, shape_id: *const u32, n_add: u32, first_index_out: *mut u32)
        -> c_int;
    pub fn xpbd_world_raycast_masked(w: *mut XpbdWorld, rays: *const XpbdRay, n_rays: u32, flags: u32, mask: u32, hits: *mut XpbdRayHit)
        -> c_int;
    pub fn xpbd_world_raycast_masked_device(w: *mut XpbdWorld, dev_rays: *const XpbdRay, n_rays: u32, flags: u32, mask: u32,
                                            dev_hits: *mut XpbdRayHit) -> c_int;
    pub fn xpbd_multi_world_raycast_masked(mw: *mut XpbdMultiWorld, rays: *const XpbdRay, n_rays: u32, flags: u32, mask: u32,
                                           hits: *mut XpbdRayHit) -> c_int;
    pub fn xpbd_world_overlap(w: *mut XpbdWorld, queries: *const XpbdOverlapQuery, n_queries: u32, flags: u32, offsets: *mut u32,
                              hits: *mut XpbdOverlapHit, cap: u32, n_out: *mut u32) -> c_int;
    pub fn xpbd_world_overlap_device(w: *mut XpbdWorld, dev_queries: *const XpbdOverlapQuery, n_queries: u32, flags: u32, dev_offsets: *mut u32,
                                     dev_hits: *mut XpbdOverlapHit, cap: u32) -> c_int;
    pub fn xpbd_multi_world_overlap(mw: *mut XpbdMultiWorld, queries: *const XpbdOverlapQuery, n_queries: u32, flags: u32, offsets: *mut u32,
                                    hits: *mut XpbdOverlapHit, cap: u32, n_out: *mut u32) -> c_int;
    pub fn xpbd_world_sweep(w: *mut XpbdWorld, sweeps: *const XpbdSweep, n_sweeps: u32, flags: u32, hits: *mut XpbdSweepHit) -> c_int;
    pub fn xpbd_world_sweep_device(w: *mut XpbdWorld, dev_sweeps: *const XpbdSweep, n_sweeps: u32, flags: u32,
                                   dev_hits: *mut XpbdSweepHit) -> c_int;
    pub fn xpbd_multi_world_sweep(mw: *mut XpbdMultiWorld, sweeps: *const XpbdSweep, n_sweeps: u32, flags: u32,
                                  hits: *mut XpbdSweepHit) -> c_int;
    pub fn xpbd_world_distance(w: *mut XpbdWorld, queries: *const XpbdDistanceQuery, n_queries: u32, flags: u32,
                               hits: *mut XpbdDistanceHit) -> c_int;
    pub fn xpbd_world_distance_device(w: *mut XpbdWorld, dev_queries: *const XpbdDistanceQuery, n_queries: u32, flags: u32,
                                      dev_hits: *mut XpbdDistanceHit) -> c_int;
    pub fn xpbd_multi_world_distance(mw: *mut XpbdMultiWorld, queries: *const XpbdDistanceQuery, n_queries: u32, flags: u32,
                                     hits: *mut XpbdDistanceHit) -> c_int;
    // the nearest feature of the terrain's surface (body = XPBD_HIT_TERRAIN); a call of its own, XPBD_QUERY_TERRAIN stays unknown
    pub fn xpbd_world_terrain_distance(w: *mut XpbdWorld, queries: *const XpbdDistanceQuery, n_queries: u32, flags: u32,
                                       hits: *mut XpbdDistanceHit) -> c_int;
    pub fn xpbd_world_terrain_distance_device(w: *mut XpbdWorld, dev_queries: *const XpbdDistanceQuery, n_queries: u32, flags: u32,
                                              dev_hits: *mut XpbdDistanceHit) -> c_int;
    pub fn xpbd_world_set_contact_report(w: *mut XpbdWorld, enable: u32) -> c_int;
    pub fn xpbd_world_contact_report_counts(w: *mut XpbdWorld, out: *mut u32) -> c_int;
    pub fn xpbd_world_download_pair_contacts(w: *mut XpbdWorld, pairs: *mut XpbdPairContact, pair_cap: u32, points: *mut XpbdContactPoint,
                                             point_cap: u32, n_pairs: *mut u32, n_points: *mut u32) -> c_int;
    pub fn xpbd_world_download_contact_events(w: *mut XpbdWorld, out: *mut XpbdContactEvent, cap: u32, n_out: *mut u32) -> c_int;
    pub fn xpbd_world_islands(w: *mut XpbdWorld, flags: u32, island_of: *mut u32, islands: *mut XpbdIsland, cap: u32,
                              n_islands: *mut u32) -> c_int;
    pub fn xpbd_world_islands_device(w: *mut XpbdWorld, flags: u32, dev_island_of: *mut u32, dev_islands: *mut XpbdIsland, cap: u32,
                                     dev_n_islands: *mut u32) -> c_int;
    // island sleeping (include/xpbd.h, "SLEEPING"); cfg NULL: off; any array of the state calls may be NULL, counts: [u32; 4]
    pub fn xpbd_world_set_sleeping(w: *mut XpbdWorld, cfg: *const XpbdSleepConfig) -> c_int;
    pub fn xpbd_world_sleep_state(w: *mut XpbdWorld, asleep: *mut u8, rest_frames: *mut u32, group: *mut u32, counts: *mut u32) -> c_int;
    pub fn xpbd_world_sleep_state_device(w: *mut XpbdWorld, dev_asleep: *mut u8, dev_rest_frames: *mut u32, dev_group: *mut u32,
                                         dev_counts: *mut u32) -> c_int;
    pub fn xpbd_world_wake_bodies(w: *mut XpbdWorld, indices: *const u32, n: u32) -> c_int;
    pub fn xpbd_world_wake_bodies_device(w: *mut XpbdWorld, dev_indices: *const u32, n: u32) -> c_int;
    // joint states and drive targets (include/xpbd.h, "Joint STATES and drive TARGETS"); a NULL list names all joints / drives
    pub fn xpbd_world_joint_states(w: *mut XpbdWorld, joints: *const u32, n: u32, out: *mut XpbdJointState) -> c_int;
    pub fn xpbd_world_joint_states_device(w: *mut XpbdWorld, dev_joints: *const u32, n: u32, dev_out: *mut XpbdJointState) -> c_int;
    pub fn xpbd_world_set_drive_targets(w: *mut XpbdWorld, drives: *const u32, targets: *const f64, n: u32) -> c_int;
    pub fn xpbd_world_set_drive_targets_device(w: *mut XpbdWorld, dev_drives: *const u32, dev_targets: *const f64, n: u32) -> c_int;
    // kinematic bodies (include/xpbd.h, "KINEMATIC bodies"); a NULL entry list names all entries; rows are [n][7] doubles
    pub fn xpbd_world_set_kinematics(w: *mut XpbdWorld, list: *const XpbdKinematic, n: u32) -> c_int;
    pub fn xpbd_world_set_kinematic_targets(w: *mut XpbdWorld, entries: *const u32, rows: *const f64, n: u32) -> c_int;
    pub fn xpbd_world_set_kinematic_targets_device(w: *mut XpbdWorld, dev_entries: *const u32, dev_rows: *const f64, n: u32) -> c_int;
    pub fn xpbd_world_kinematic_count(w: *const XpbdWorld) -> u32;
    // sensor bodies (include/xpbd.h, "SENSOR bodies"): one byte per body (NULL with n = 0 clears); the occupancy of the report frame
    pub fn xpbd_world_set_sensors(w: *mut XpbdWorld, is_sensor: *const u8, n: u32) -> c_int;
    pub fn xpbd_world_get_sensors(w: *mut XpbdWorld, is_sensor: *mut u8, n: u32) -> c_int;
    pub fn xpbd_world_sensor_count(w: *const XpbdWorld) -> u32;
    pub fn xpbd_world_sensor_overlaps(w: *mut XpbdWorld, sensors: *mut u32, offsets: *mut u32, hits: *mut XpbdSensorHit, cap: u32,
                                      n_out: *mut u32) -> c_int;
    pub fn xpbd_world_sensor_overlaps_device(w: *mut XpbdWorld, dev_sensors: *mut u32, dev_offsets: *mut u32, dev_hits: *mut XpbdSensorHit,
                                             cap: u32) -> c_int;
    // mass edits (include/xpbd.h, "MASS properties of resident bodies"); a NULL index list names all bodies; rows are [n][13] doubles
    pub fn xpbd_world_set_mass_properties(w: *mut XpbdWorld, indices: *const u32, n: u32, rows: *const f64, flags: u32) -> c_int;
    pub fn xpbd_world_set_mass_properties_device(w: *mut XpbdWorld, dev_indices: *const u32, n: u32, dev_rows: *const f64, flags: u32) -> c_int;
    pub fn xpbd_world_get_mass_properties(w: *mut XpbdWorld, indices: *const u32, n: u32, rows: *mut f64) -> c_int;
    pub fn xpbd_multi_world_set_contact_report(mw: *mut XpbdMultiWorld, enable: u32) -> c_int;
    pub fn xpbd_multi_world_contact_report_counts(mw: *mut XpbdMultiWorld, out: *mut u32) -> c_int;
    pub fn xpbd_multi_world_download_pair_contacts(mw: *mut XpbdMultiWorld, pairs: *mut XpbdPairContact, pair_cap: u32,
                                                   points: *mut XpbdContactPoint, point_cap: u32, n_pairs: *mut u32, n_points: *mut u32)
        -> c_int;
    pub fn xpbd_multi_world_download_contact_events(mw: *mut XpbdMultiWorld, out: *mut XpbdContactEvent, cap: u32, n_out: *mut u32) -> c_int;
}

fn v3(v: Vector3<f64>) -> [f64; 3] {
    [v.x, v.y, v.z]
}

fn from3(a: [f64; 3]) -> Vector3<f64> {
    Vector3::new(a[0], a[1], a[2])
}

impl From<&Rigid> for XpbdRigid {
    fn from(r: &Rigid) -> Self {
        let m: &Matrix3<f64> = &r.inverse_inertia;
        XpbdRigid {
            inverse_mass: r.inverse_mass,
            inverse_inertia: [m.x.x, m.x.y, m.x.z, m.y.x, m.y.y, m.y.z, m.z.x, m.z.y, m.z.z],
            external_force: v3(r.external_force),
            internal_force: v3(r.internal_force),
            external_torque: v3(r.external_torque),
            internal_torque: v3(r.internal_torque),
            velocity: v3(r.velocity),
            angular_velocity: v3(r.angular_velocity),
            center_of_mass: v3(r.center_of_mass),
            position: v3(r.position),
            rotation: [r.rotation.s, r.rotation.v.x, r.rotation.v.y, r.rotation.v.z],
        }
    }
}

impl XpbdRigid {
    /// Writes the dynamic state back; the static fields were never changed by the device.
    pub fn store_into(&self, r: &mut Rigid) {
        r.velocity = from3(self.velocity);
        r.angular_velocity = from3(self.angular_velocity);
        r.position = from3(self.position);
        r.rotation = Quaternion::new(self.rotation[0], self.rotation[1], self.rotation[2], self.rotation[3]);
    }
}

fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { CStr::from_ptr(xpbd_last_error()) }.to_string_lossy().into_owned();
        // the reference panics on its own failure paths (src/rigid.rs:59); keep that contract
        panic!("xpbd error {}: {}", rc, msg);
    }
}

fn flat_vertices(polytope: &Polytope) -> Vec<f64> {
    polytope.vertices.iter().flat_map(|v| [v.x, v.y, v.z]).collect()
}

/// Drop-in body for `solver::step` (src/solver.rs:3): same signature, same result.
pub fn step(rigid: &mut Rigid, polytope: &Polytope, dt: f64, substep_count: usize) {
    let mut c = XpbdRigid::from(&*rigid);
    let verts = flat_vertices(polytope);
    check(unsafe { xpbd_step_one(&mut c, verts.as_ptr(), polytope.vertices.len() as u32, dt, substep_count as u32) });
    c.store_into(rigid);
}

/// N-body world resident on one GPU: upload once, `integrate` every frame, read poses back for rendering.
pub struct GpuWorld {
    handle: *mut XpbdWorld,
    staging: Vec<XpbdRigid>,
}

impl GpuWorld {
    pub fn new(device: i32, shapes: &[&Polytope], bodies: &[Rigid], shape_id: &[u32]) -> GpuWorld {
        let mut cfg = XpbdConfig::default();
        unsafe { xpbd_config_default(&mut cfg) };
        cfg.device = device;
        let mut handle = std::ptr::null_mut();
        check(unsafe { xpbd_world_create(&mut handle, &cfg) });
        let mut verts = Vec::new();
        let mut offsets = vec![0u32];
        for p in shapes {
            verts.extend(flat_vertices(p));
            offsets.push((verts.len() / 3) as u32);
        }
        check(unsafe { xpbd_world_set_shapes(handle, verts.as_ptr(), offsets.as_ptr(), shapes.len() as u32) });
        let staging: Vec<XpbdRigid> = bodies.iter().map(XpbdRigid::from).collect();
        check(unsafe { xpbd_world_upload_bodies(handle, staging.as_ptr(), shape_id.as_ptr(), staging.len() as u32) });
        GpuWorld { handle, staging }
    }

    /// World::integrate (src/world.rs:34-43) for every body: solver::step(body, shape, dt, substeps).
    pub fn integrate(&mut self, dt: f64, substeps: u32) {
        check(unsafe { xpbd_world_step(self.handle, dt, substeps) });
    }

    /// Read-back for rendering (src/app.rs:227-230 consumes Rigid::frame()).
    pub fn read_back(&mut self, bodies: &mut [Rigid]) {
        check(unsafe { xpbd_world_download_bodies(self.handle, self.staging.as_mut_ptr(), self.staging.len() as u32) });
        for (c, r) in self.staging.iter().zip(bodies.iter_mut()) {
            c.store_into(r);
        }
    }
}

/// The app's state history (src/app.rs:48, 206-212) on the device: `states` becomes the world's history,
/// `current_state` stays a host-side cursor.  `advance` is the body of the `RedrawRequested` loop.
pub struct Timeline {
    pub world: GpuWorld,
    pub current_state: u32,
}

impl Timeline {
    /// `states = vec![(World::new(..), ..)]; current_state = 0`
    pub fn new(world: GpuWorld) -> Timeline {
        check(unsafe { xpbd_world_history_push(world.handle, std::ptr::null_mut()) });
        Timeline { world, current_state: 0 }
    }

    /// `for _ in 0..time_speed() { if current_state + 1 >= states.len() { integrate; push } current_state += 1 }`
    pub fn advance(&mut self, dt: f64, substeps: u32, time_speed: u32) {
        for _ in 0..time_speed {
            let len = unsafe { xpbd_world_history_length(self.world.handle) };
            if self.current_state + 1 >= len {
                check(unsafe { xpbd_world_history_restore(self.world.handle, len - 1) });
                self.world.integrate(dt, substeps);
                check(unsafe { xpbd_world_history_push(self.world.handle, std::ptr::null_mut()) });
            }
            self.current_state += 1;
        }
    }

    /// Scrubbing: show state `index` (the renderer then calls `world.read_back`).
    pub fn seek(&mut self, index: u32) {
        check(unsafe { xpbd_world_history_restore(self.world.handle, index) });
        self.current_state = index;
    }
}

impl Drop for GpuWorld {
    fn drop(&mut self) {
        unsafe { xpbd_world_destroy(self.handle) };
    }
}
