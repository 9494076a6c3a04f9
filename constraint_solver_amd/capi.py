"""ctypes binding of the C ABI (include/xpbd.h) and of the host mirror's C window.

Test / bench glue only: the product is the shared library.  There is no Python or
CPU fallback -- if libxpbd_hip.so is missing the import fails, and without a GPU
every compute call returns an error that is raised as XpbdError.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_PKG, "lib")

RIGID_DOUBLES = 38
BYTES_PER_BODY_SUBSTEP = 412  # read 13+25 doubles + 4 B shape id, write 13 doubles

MODE_FUSED = 0
MODE_PER_SUBSTEP = 1
MODE_CONTACTS = 2  # extension: ground + body-body contacts
FLAG_TRACE_CONTACTS = 1

OK, E_INVALID, E_HIP, E_OOM, E_SINGULAR_INERTIA, E_NO_DEVICE, E_CAPACITY, E_HALO = 0, -1, -2, -3, -4, -5, -6, -7

# xpbd_rigid field -> (first double, count); order of reference src/rigid.rs:6-50
RIGID_FIELDS = {
    "inverse_mass": (0, 1), "inverse_inertia": (1, 9), "external_force": (10, 3), "internal_force": (13, 3),
    "external_torque": (16, 3), "internal_torque": (19, 3), "velocity": (22, 3), "angular_velocity": (25, 3),
    "center_of_mass": (28, 3), "position": (31, 3), "rotation": (34, 4),
}

# Every symbol include/xpbd.h declares (tests check the library exports all of them).
ABI_SYMBOLS = [
    "xpbd_abi_version", "xpbd_last_error", "xpbd_config_default", "xpbd_device_count", "xpbd_world_create",
    "xpbd_world_destroy", "xpbd_world_set_shapes", "xpbd_world_upload_bodies", "xpbd_world_download_bodies",
    "xpbd_world_body_count", "xpbd_world_download_frames", "xpbd_world_step", "xpbd_world_synchronize", "xpbd_world_download_contacts",
    "xpbd_world_download_contact_masks", "xpbd_world_set_stream", "xpbd_world_get_stream", "xpbd_world_set_mode",
    "xpbd_step_one", "xpbd_selftest_div_sqrt", "xpbd_selftest_exact_math", "xpbd_world_set_polytopes", "xpbd_world_narrowphase",
    "xpbd_world_set_contact_pad", "xpbd_world_set_max_depenetration_speed", "xpbd_multi_world_set_max_depenetration_speed",
    "xpbd_world_contact_stats", "xpbd_world_build_neighbours",
    "xpbd_world_download_neighbours", "xpbd_world_contacts_begin", "xpbd_world_contacts_substep",
    "xpbd_world_export_dynamic", "xpbd_world_import_dynamic", "xpbd_world_import_dynamic_rows", "xpbd_world_set_joints",
    "xpbd_world_set_joint_limits", "xpbd_multi_world_set_joint_limits",
    "xpbd_world_set_joint_drives", "xpbd_multi_world_set_joint_drives",
    "xpbd_world_narrowphase_gjk", "xpbd_world_set_narrowphase",
    "xpbd_world_set_sat_schedule",
    "xpbd_world_edge_axes_separation",
    "xpbd_selftest_hbm_copy", "xpbd_selftest_field_streams", "xpbd_selftest_gather", "xpbd_world_snapshot_positions", "xpbd_world_max_displacement2",
    "xpbd_comm_unique_id", "xpbd_comm_library", "xpbd_multi_config_default", "xpbd_multi_world_create", "xpbd_multi_world_destroy",
    "xpbd_multi_world_set_polytopes", "xpbd_multi_world_upload", "xpbd_multi_world_step", "xpbd_multi_world_replan",
    "xpbd_multi_world_synchronize", "xpbd_multi_world_download", "xpbd_multi_world_halo_stats", "xpbd_multi_world_contact_stats",
    "xpbd_halo_cell_key", "xpbd_halo_plan", "xpbd_halo_plan_far", "xpbd_halo_partition", "xpbd_halo_plan_owned", "xpbd_halo_plan_light",
    "xpbd_multi_world_download_owned", "xpbd_multi_world_plan_stats", "xpbd_multi_world_owners",
    "xpbd_world_history_push", "xpbd_world_history_restore", "xpbd_world_history_truncate", "xpbd_world_history_length",
    "xpbd_world_raycast", "xpbd_world_raycast_device", "xpbd_multi_world_raycast",
    "xpbd_world_set_collision_filters", "xpbd_multi_world_set_collision_filters", "xpbd_world_raycast_masked",
    "xpbd_world_raycast_masked_device", "xpbd_multi_world_raycast_masked",
    "xpbd_world_set_contact_report", "xpbd_world_contact_report_counts", "xpbd_world_download_pair_contacts",
    "xpbd_world_download_contact_events", "xpbd_multi_world_set_contact_report", "xpbd_multi_world_contact_report_counts",
    "xpbd_multi_world_download_pair_contacts", "xpbd_multi_world_download_contact_events",
    "xpbd_world_set_materials", "xpbd_multi_world_set_materials", "xpbd_world_set_restitution",
    "xpbd_world_set_external_wrench", "xpbd_world_set_external_wrench_device", "xpbd_world_apply_impulses",
    "xpbd_world_apply_impulses_device", "xpbd_world_set_dynamics", "xpbd_world_get_dynamics",
    "xpbd_multi_world_set_external_wrench", "xpbd_multi_world_apply_impulses",
    "xpbd_world_overlap", "xpbd_world_overlap_device", "xpbd_multi_world_overlap",
    "xpbd_world_sweep", "xpbd_world_sweep_device", "xpbd_multi_world_sweep",
    "xpbd_world_distance", "xpbd_world_distance_device", "xpbd_multi_world_distance",
    "xpbd_world_terrain_distance", "xpbd_world_terrain_distance_device",
    "xpbd_world_remove_bodies", "xpbd_world_remove_bodies_device", "xpbd_world_add_bodies",
    "xpbd_world_set_terrain", "xpbd_world_sample_terrain",
    "xpbd_world_islands", "xpbd_world_islands_device",
    "xpbd_world_set_sleeping", "xpbd_world_sleep_state", "xpbd_world_sleep_state_device", "xpbd_world_wake_bodies",
    "xpbd_world_wake_bodies_device",
    "xpbd_world_joint_states", "xpbd_world_joint_states_device", "xpbd_world_set_drive_targets", "xpbd_world_set_drive_targets_device",
    "xpbd_world_set_kinematics", "xpbd_world_set_kinematic_targets", "xpbd_world_set_kinematic_targets_device", "xpbd_world_kinematic_count",
    "xpbd_world_set_mass_properties", "xpbd_world_set_mass_properties_device", "xpbd_world_get_mass_properties",
    "xpbd_world_set_damping", "xpbd_world_get_damping", "xpbd_world_set_joint_damping",
    "xpbd_world_set_sensors", "xpbd_world_get_sensors", "xpbd_world_sensor_count", "xpbd_world_sensor_overlaps", "xpbd_world_sensor_overlaps_device",
]

# sensor bodies (include/xpbd.h, "SENSOR bodies"): xpbd_sensor_hit, 8 bytes
SENSOR_HIT_DTYPE = np.dtype([("body", "<u4"), ("pair", "<u4")])

# damping (include/xpbd.h, "DAMPING"): xpbd_body_damping, 32 bytes, and xpbd_joint_damping, 24 bytes
BODY_DAMPING_DTYPE = np.dtype([("linear", np.float64), ("angular", np.float64), ("max_linear_speed", np.float64), ("max_angular_speed", np.float64)])
JOINT_DAMPING_DTYPE = np.dtype([("joint", np.uint32), ("reserved", np.uint32), ("linear", np.float64), ("angular", np.float64)])


def body_damping(n, linear=0.0, angular=0.0, max_linear_speed=np.inf, max_angular_speed=np.inf):
    """n BODY_DAMPING_DTYPE rows; every argument a scalar or an array of n.  The defaults are the default row."""
    rows = np.zeros(n, dtype=BODY_DAMPING_DTYPE)
    rows["linear"], rows["angular"], rows["max_linear_speed"], rows["max_angular_speed"] = linear, angular, max_linear_speed, max_angular_speed
    return rows


def joint_damping(joint, linear=0.0, angular=0.0):
    """JOINT_DAMPING_DTYPE records for the joints `joint` (an array); linear, angular: scalars or arrays of the same length."""
    joint = np.asarray(joint, dtype=np.uint32).reshape(-1)
    out = np.zeros(joint.size, dtype=JOINT_DAMPING_DTYPE)
    out["joint"], out["linear"], out["angular"] = joint, linear, angular
    return out

# mass edits (include/xpbd.h, "MASS properties of resident bodies"): the flags, and the doubles of a row
MASS_INVERSE, MASS_DIRECT, MASS_KEEP_FRAME = 0, 1, 0x100
MASS_DOUBLES = 13                 # inverse_mass | mass, inverse_inertia[9] | inertia[9] (column-major), center_of_mass[3]

# kinematic bodies (include/xpbd.h, "KINEMATIC bodies"): xpbd_kinematic, 64 bytes
KINEMATIC_POSE, KINEMATIC_VELOCITY = 0, 1
KINEMATIC_DTYPE = np.dtype([("body", np.uint32), ("mode", np.uint32), ("linear", np.float64, 3), ("angular", np.float64, 4)])


def kinematics(body, mode, linear, angular):
    """KINEMATIC_DTYPE records: POSE entries take a target position and rotation (s, x, y, z), VELOCITY entries a velocity and
    an angular velocity (three components; a fourth is ignored)."""
    body = np.atleast_1d(np.asarray(body, dtype=np.uint32))
    out = np.zeros(body.size, dtype=KINEMATIC_DTYPE)
    out["body"] = body
    out["mode"] = mode
    out["linear"] = np.asarray(linear, dtype=np.float64).reshape(-1, 3)
    ang = np.asarray(angular, dtype=np.float64)
    ang = ang.reshape(-1, ang.shape[-1])
    out["angular"][:, :ang.shape[1]] = ang
    return out


class XpbdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("xpbd error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("mode", C.c_uint32), ("flags", C.c_uint32),
                ("block_size", C.c_uint32), ("reserved", C.c_uint32 * 3)]


_u32p = C.POINTER(C.c_uint32)
_f64p = C.POINTER(C.c_double)


class MultiConfig(C.Structure):
    """xpbd_multi_config"""
    _fields_ = [("struct_size", C.c_uint32), ("n_ranks", C.c_uint32), ("first_rank", C.c_uint32), ("n_local", C.c_uint32),
                ("devices", C.POINTER(C.c_int32)), ("transport", C.c_uint32), ("flags", C.c_uint32), ("comm_id", C.c_char_p),
                ("contact_pad", C.c_double), ("halo_margin", C.c_double), ("narrowphase", C.c_uint32), ("reserved", C.c_uint32)]


class HEIGHTFIELD(C.Structure):
    """xpbd_heightfield (48 bytes): terrain (EXTENSION)"""
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("origin", C.c_double * 2), ("cell", C.c_double * 2), ("heights", _f64p)]


MAX_TERRAIN_SAMPLES = 1 << 22
COMM_ID_BYTES = 128
TRANSPORT_RCCL, TRANSPORT_LOCAL = 0, 1
MULTI_AUTO_REPLAN = 1
MULTI_PLAN_THROUGH_DEVICE = 2
MULTI_FULL_PLANS = 8


class PolytopeDesc(C.Structure):
    """xpbd_polytope"""
    _fields_ = [("vertices_xyz", _f64p), ("edges", _u32p), ("face_offsets", _u32p), ("face_indices", _u32p),
                ("n_vertices", C.c_uint32), ("n_edges", C.c_uint32), ("n_faces", C.c_uint32), ("reserved", C.c_uint32),
                ("centroid", C.c_double * 3)]


# xpbd_joint as a numpy record (120 bytes)
JOINT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("anchor_a", "<f8", (3,)), ("anchor_b", "<f8", (3,)),
                        ("distance", "<f8"), ("axis_a", "<f8", (3,)), ("axis_b", "<f8", (3,)), ("kind", "<u4"), ("reserved", "<u4")])
JOINT_DISTANCE, JOINT_HINGE, JOINT_SLIDER = 0, 1, 2
# xpbd_joint_limit as a numpy record (72 bytes)
JOINT_LIMIT_DTYPE = np.dtype([("joint", "<u4"), ("kind", "<u4"), ("ref_a", "<f8", (3,)), ("ref_b", "<f8", (3,)),
                              ("lower", "<f8"), ("upper", "<f8")])
LIMIT_HINGE, LIMIT_SWING, LIMIT_TWIST, LIMIT_SLIDE = 0, 1, 2, 3
# xpbd_joint_drive as a numpy record (80 bytes)
JOINT_DRIVE_DTYPE = np.dtype([("joint", "<u4"), ("kind", "<u4"), ("ref_a", "<f8", (3,)), ("ref_b", "<f8", (3,)),
                              ("target", "<f8"), ("compliance", "<f8"), ("max_force", "<f8")])
DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY, DRIVE_POSITION, DRIVE_VELOCITY = 0, 1, 2, 3
# xpbd_joint_state as a numpy record (80 bytes): what World.joint_states reports of one joint; XPBD_JOINT_STATE_* flags
JOINT_STATE_DTYPE = np.dtype([("separation", "<f8"), ("misalignment", "<f8"), ("angle", "<f8"), ("angle_rate", "<f8"), ("travel", "<f8"),
                              ("travel_rate", "<f8"), ("swing", "<f8"), ("twist", "<f8"), ("joint", "<u4"), ("kind", "<u4"), ("flags", "<u4"),
                              ("reserved", "<u4")])
JOINT_STATE_HAS_ANGLE, JOINT_STATE_HAS_TRAVEL, JOINT_STATE_HAS_SWING, JOINT_STATE_HAS_TWIST = 0x001, 0x002, 0x004, 0x008
JOINT_STATE_ANGLE_OF_DRIVE = 0x010   # angle, angle_rate use the angular drive's references (else the hinge limit's)
JOINT_STATE_ANGLE_BELOW, JOINT_STATE_ANGLE_ABOVE, JOINT_STATE_TRAVEL_BELOW, JOINT_STATE_TRAVEL_ABOVE = 0x100, 0x200, 0x400, 0x800
JOINT_STATE_SWING_ABOVE, JOINT_STATE_TWIST_BELOW, JOINT_STATE_TWIST_ABOVE = 0x1000, 0x2000, 0x4000
JOINT_STATE_NO_JOINT = 0xFFFFFFFF    # .kind of an index out of range (device variant)
# xpbd_collision_filter as a numpy record (8 bytes): bodies i, j may touch iff group_i & mask_j and group_j & mask_i
COLLISION_FILTER_DTYPE = np.dtype([("group", "<u4"), ("mask", "<u4")])
FILTER_JOINTED = 1                # bodies joined by a joint never collide
# xpbd_material as a numpy record (16 bytes): Coulomb friction coefficient >= 0 (+inf: the reference's contact), reserved = 0
MATERIAL_DTYPE = np.dtype([("friction", "<f8"), ("reserved", "<f8")])
# body edits (EXTENSION): xpbd_impulse as a ctypes struct and as a numpy record (80 bytes)
IMPULSE_AT_POINT, IMPULSE_AT_CENTRE = 0, 1
DYNAMIC_DOUBLES = 13              # a row of set_dynamics / get_dynamics: position, rotation {s,x,y,z}, velocity, angular_velocity


class Impulse(C.Structure):
    """xpbd_impulse"""
    _fields_ = [("body", C.c_uint32), ("flags", C.c_uint32), ("impulse", C.c_double * 3), ("point", C.c_double * 3),
                ("angular_impulse", C.c_double * 3)]


IMPULSE_DTYPE = np.dtype([("body", "<u4"), ("flags", "<u4"), ("impulse", "<f8", (3,)), ("point", "<f8", (3,)),
                          ("angular_impulse", "<f8", (3,))])
# xpbd_gjk_result as a numpy record (96 bytes)
GJK_DTYPE = np.dtype([("status", "<i4"), ("gjk_iterations", "<u4"), ("epa_iterations", "<u4"), ("reserved", "<u4"),
                      ("depth", "<f8"), ("normal", "<f8", (3,)), ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,))])
GJK_SEPARATED, GJK_PENETRATING, GJK_DEGENERATE = 0, 1, 2
# xpbd_edge_query as a numpy record (16 bytes)
EDGE_QUERY_DTYPE = np.dtype([("separation", "<f8"), ("edge_a", "<u4"), ("edge_b", "<u4")])
NARROWPHASE_SAT, NARROWPHASE_GJK_EPA = 0, 1
MAX_MANIFOLD_POINTS = 8
FEATURE_FACE_A, FEATURE_FACE_B, FEATURE_EDGES = 0, 1, 2
# xpbd_manifold as a numpy record (408 bytes)
# xpbd_ray / xpbd_ray_hit as numpy records (64 bytes each); scene queries (EXTENSION)
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("max_distance", "<f8"), ("ignore_body", "<u4"),
                      ("reserved", "<u4")])
RAY_HIT_DTYPE = np.dtype([("body", "<u4"), ("face", "<u4"), ("distance", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,))])
NO_HIT = RAY_INSIDE = 0xFFFFFFFF
RAYCAST_BRUTE_FORCE = 1
RAYCAST_BRUTE_FORCE_RAYS = 8      # calls with at most this many rays take the brute-force path anyway
# Terrain in the scene queries (EXTENSION): a flag of raycast, overlap and sweep alike (World only; MultiWorld has no terrain)
QUERY_TERRAIN = 0x100             # the heightfield of World.set_terrain answers too
HIT_TERRAIN = 0xFFFFFFFE          # .body of a hit on the terrain; .face is then the triangle 2 * (j * (nx - 1) + i) + k


def rays(origins, directions, max_distance=np.inf, ignore=None):
    """RAY_DTYPE records from (n, 3) origins and directions (broadcast), a max_distance per ray or for all, and the body each
    ray ignores (None: none)."""
    o, d = np.atleast_2d(np.asarray(origins, dtype=np.float64)), np.atleast_2d(np.asarray(directions, dtype=np.float64))
    n = max(o.shape[0], d.shape[0])
    out = np.zeros(n, dtype=RAY_DTYPE)
    out["origin"], out["direction"], out["max_distance"] = o, d, max_distance
    out["ignore_body"] = NO_HIT if ignore is None else ignore
    return out


# xpbd_overlap_query (72 bytes) / xpbd_overlap_hit (16 bytes) as numpy records; overlap queries (EXTENSION)
OVERLAP_QUERY_DTYPE = np.dtype([("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("shape", "<u4"), ("ignore_body", "<u4"),
                                ("mask", "<u4"), ("reserved", "<u4")])
OVERLAP_HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("separation", "<f8")])
OVERLAP_BRUTE_FORCE, OVERLAP_MASKED = 1, 2
OVERLAP_SORT_STAGE = 1024         # hits of one query the sort stages in LDS (kOverlapSortStage, csrc/xpbd_query.h)


def overlap_queries(position, rotation, shape, ignore=None, mask=None):
    """OVERLAP_QUERY_DTYPE records from (n, 3) positions, (n, 4) rotations {s, x, y, z} and shape indices (all broadcast), the
    body each query ignores (None: none) and its group mask (None: ~0; read with OVERLAP_MASKED only)."""
    p, r = np.atleast_2d(np.asarray(position, dtype=np.float64)), np.atleast_2d(np.asarray(rotation, dtype=np.float64))
    sh = np.atleast_1d(np.asarray(shape, dtype=np.uint32))
    extra = [np.atleast_1d(np.asarray(x)) for x in (ignore, mask) if x is not None]
    n = max([p.shape[0], r.shape[0], sh.shape[0]] + [x.shape[0] for x in extra])
    out = np.zeros(n, dtype=OVERLAP_QUERY_DTYPE)
    out["position"], out["rotation"], out["shape"] = p, r, sh
    out["ignore_body"] = NO_HIT if ignore is None else ignore
    out["mask"] = 0xFFFFFFFF if mask is None else mask
    return out


def _overlap(fn, h, queries, flags):
    """(offsets, hits) of an overlap call with host arrays: once to count, once to fill."""
    q = np.ascontiguousarray(queries, dtype=OVERLAP_QUERY_DTYPE).reshape(-1)
    offsets = np.zeros(q.size + 1, dtype=np.uint32)
    total = C.c_uint32(0)
    qp = q.ctypes.data if q.size else None
    rc = fn(h, qp, q.size, flags, offsets.ctypes.data, None, 0, C.byref(total))
    if rc != E_CAPACITY:            # (a count of more than nothing comes back as "no room")
        _check(rc)
    hits = np.zeros(total.value, dtype=OVERLAP_HIT_DTYPE)
    if total.value:
        _check(fn(h, qp, q.size, flags, offsets.ctypes.data, hits.ctypes.data, hits.size, C.byref(total)))
    return offsets, hits


# xpbd_sweep (104 bytes) / xpbd_sweep_hit (72 bytes) as numpy records; sweep queries (EXTENSION)
SWEEP_DTYPE = np.dtype([("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("direction", "<f8", (3,)), ("max_distance", "<f8"),
                        ("shape", "<u4"), ("ignore_body", "<u4"), ("mask", "<u4"), ("reserved", "<u4")])
SWEEP_HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("face", "<u4"), ("reserved", "<u4"), ("distance", "<f8"),
                            ("position", "<f8", (3,)), ("normal", "<f8", (3,))])
SWEEP_INITIAL = 3                 # xpbd_sweep_hit.feature: the volume overlaps the body at t = 0
SWEEP_BRUTE_FORCE, SWEEP_MASKED = 1, 2
SWEEP_BRUTE_FORCE_SWEEPS = 8      # calls with at most this many sweeps take the brute-force path anyway


def sweeps(position, rotation, direction, shape, max_distance=np.inf, ignore=None, mask=None):
    """SWEEP_DTYPE records from (n, 3) positions, (n, 4) rotations {s, x, y, z}, (n, 3) directions and shape indices (all
    broadcast), a max_distance per sweep or for all, the body each sweep ignores (None: none) and its group mask (None: ~0; read
    with SWEEP_MASKED only)."""
    p, r = np.atleast_2d(np.asarray(position, dtype=np.float64)), np.atleast_2d(np.asarray(rotation, dtype=np.float64))
    d, sh = np.atleast_2d(np.asarray(direction, dtype=np.float64)), np.atleast_1d(np.asarray(shape, dtype=np.uint32))
    extra = [np.atleast_1d(np.asarray(x)) for x in (max_distance, ignore, mask) if x is not None]
    n = max([p.shape[0], r.shape[0], d.shape[0], sh.shape[0]] + [x.shape[0] for x in extra])
    out = np.zeros(n, dtype=SWEEP_DTYPE)
    out["position"], out["rotation"], out["direction"], out["shape"], out["max_distance"] = p, r, d, sh, max_distance
    out["ignore_body"] = NO_HIT if ignore is None else ignore
    out["mask"] = 0xFFFFFFFF if mask is None else mask
    return out


def _sweep(fn, h, sweeps, flags):
    s = np.ascontiguousarray(sweeps, dtype=SWEEP_DTYPE).reshape(-1)
    out = np.zeros(s.size, dtype=SWEEP_HIT_DTYPE)
    _check(fn(h, s.ctypes.data if s.size else None, s.size, flags, out.ctypes.data if s.size else None))
    return out


# xpbd_distance_query (80 bytes) / xpbd_distance_hit (96 bytes) as numpy records; distance queries (EXTENSION)
DISTANCE_QUERY_DTYPE = np.dtype([("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("max_distance", "<f8"), ("shape", "<u4"),
                                 ("ignore_body", "<u4"), ("mask", "<u4"), ("reserved", "<u4")])
DISTANCE_HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("index_a", "<u4"), ("index_b", "<u4"), ("distance", "<f8"),
                               ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,)), ("normal", "<f8", (3,))])
DISTANCE_BRUTE_FORCE, DISTANCE_MASKED = 1, 2
DISTANCE_OVERLAP = 3              # xpbd_distance_hit.feature: the volume and the body are not separated (distance 0)
DISTANCE_POINT = 0xFFFFFFFF       # xpbd_distance_query.shape: the volume is the single point `position`
DISTANCE_BRUTE_FORCE_QUERIES = 8  # calls with at most this many queries take the brute-force path anyway


def distances(position, rotation=(1.0, 0.0, 0.0, 0.0), shape=DISTANCE_POINT, max_distance=np.inf, ignore=None, mask=None):
    """DISTANCE_QUERY_DTYPE records from (n, 3) positions, (n, 4) rotations {s, x, y, z} and shape indices (all broadcast; the
    default shape is DISTANCE_POINT, the point `position`), a max_distance per query or for all, the body each query ignores
    (None: none) and its group mask (None: ~0; read with DISTANCE_MASKED only)."""
    p, r = np.atleast_2d(np.asarray(position, dtype=np.float64)), np.atleast_2d(np.asarray(rotation, dtype=np.float64))
    sh = np.atleast_1d(np.asarray(shape, dtype=np.uint32))
    extra = [np.atleast_1d(np.asarray(x)) for x in (max_distance, ignore, mask) if x is not None]
    n = max([p.shape[0], r.shape[0], sh.shape[0]] + [x.shape[0] for x in extra])
    out = np.zeros(n, dtype=DISTANCE_QUERY_DTYPE)
    out["position"], out["rotation"], out["shape"], out["max_distance"] = p, r, sh, max_distance
    out["ignore_body"] = NO_HIT if ignore is None else ignore
    out["mask"] = 0xFFFFFFFF if mask is None else mask
    return out


def _distance(fn, h, queries, flags):
    q = np.ascontiguousarray(queries, dtype=DISTANCE_QUERY_DTYPE).reshape(-1)
    out = np.zeros(q.size, dtype=DISTANCE_HIT_DTYPE)
    _check(fn(h, q.ctypes.data if q.size else None, q.size, flags, out.ctypes.data if q.size else None))
    return out


# Contact reports (EXTENSION): xpbd_pair_contact (64 bytes), xpbd_contact_point (48), xpbd_contact_event (12)
PAIR_CONTACT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("substeps", "<u4"), ("n_points", "<u4"), ("feature", "<u4"),
                               ("first_point", "<u4"), ("reserved", "<u4", (2,)), ("normal", "<f8", (3,)), ("depth", "<f8")])
CONTACT_POINT_DTYPE = np.dtype([("p_ref", "<f8", (3,)), ("p_inc", "<f8", (3,))])
CONTACT_EVENT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("kind", "<u4")])
CONTACT_BEGIN, CONTACT_END = 0, 1

# Contact islands (EXTENSION): xpbd_island (40 bytes)
ISLAND_DTYPE = np.dtype([("first_body", "<u4"), ("n_bodies", "<u4"), ("n_pairs", "<u4"), ("n_joints", "<u4"), ("n_anchors", "<u4"),
                         ("n_grounded", "<u4"), ("max_speed2", "<f8"), ("max_angular_speed2", "<f8")])
ISLAND_NONE = 0xFFFFFFFF          # island_of[] of a fixed body
ISLANDS_NO_JOINTS, ISLANDS_NO_CONTACTS = 1, 2


class SLEEP_CONFIG(C.Structure):
    """xpbd_sleep_config (24 bytes): island sleeping (EXTENSION)"""
    _fields_ = [("linear_speed", C.c_double), ("angular_speed", C.c_double), ("frames_to_sleep", C.c_uint32), ("flags", C.c_uint32)]


SLEEP_GROUP_NONE = 0xFFFFFFFF     # group[] of a body that is awake

MANIFOLD_DTYPE = np.dtype([("n_points", "<u4"), ("feature", "<u4"), ("index_a", "<u4"), ("index_b", "<u4"),
                           ("separation", "<f8"), ("p_ref", "<f8", (8, 3)), ("p_inc", "<f8", (8, 3))])


def _load(name):
    path = os.path.join(LIB_DIR, name)
    if name == "libxpbd_hip.so" and os.environ.get("XPBD_HIP_LIB"):     # A/B measurements of kernel variants (scripts/)
        path = os.environ["XPBD_HIP_LIB"]
    if not os.path.exists(path):
        raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(no CPU fallback exists)" % path)
    return C.CDLL(path)


_hip = None
_host = None


def hip_lib():
    """libxpbd_hip.so with argtypes set.  Loading works without a GPU; compute calls then fail loudly."""
    global _hip
    if _hip is None:
        L = _load("libxpbd_hip.so")
        L.xpbd_abi_version.restype = C.c_uint32
        L.xpbd_last_error.restype = C.c_char_p
        L.xpbd_config_default.argtypes = [C.POINTER(Config)]
        L.xpbd_config_default.restype = None
        L.xpbd_world_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Config)]
        L.xpbd_world_destroy.argtypes = [C.c_void_p]
        L.xpbd_world_destroy.restype = None
        L.xpbd_world_set_shapes.argtypes = [C.c_void_p, _f64p, _u32p, C.c_uint32]
        L.xpbd_world_upload_bodies.argtypes = [C.c_void_p, C.c_void_p, _u32p, C.c_uint32]
        L.xpbd_world_download_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_world_download_frames.argtypes = [C.c_void_p, _f64p, C.c_uint32]
        L.xpbd_world_body_count.argtypes = [C.c_void_p]
        L.xpbd_world_body_count.restype = C.c_uint32
        L.xpbd_world_step.argtypes = [C.c_void_p, C.c_double, C.c_uint32]
        L.xpbd_world_synchronize.argtypes = [C.c_void_p]
        L.xpbd_world_download_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
        L.xpbd_world_download_contact_masks.argtypes = [C.c_void_p, _u32p, C.c_uint32, C.c_uint32]
        L.xpbd_world_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.xpbd_world_get_stream.argtypes = [C.c_void_p]
        L.xpbd_world_get_stream.restype = C.c_void_p
        L.xpbd_world_set_mode.argtypes = [C.c_void_p, C.c_uint32]
        L.xpbd_step_one.argtypes = [C.c_void_p, _f64p, C.c_uint32, C.c_double, C.c_uint32]
        L.xpbd_selftest_div_sqrt.argtypes = [C.c_int32, _f64p, _f64p, _f64p, _f64p, C.c_uint32]
        try:
            L.xpbd_selftest_exact_math.argtypes = [C.c_int32, _f64p, _f64p, C.c_double, C.c_uint32, _f64p, _f64p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB for an A/B measurement (scripts/)
            pass
        L.xpbd_selftest_hbm_copy.argtypes = [C.c_int32, C.c_uint64, C.c_uint32, _f64p]
        L.xpbd_selftest_field_streams.argtypes = [C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, _f64p]
        L.xpbd_world_snapshot_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.xpbd_world_max_displacement2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xpbd_comm_unique_id.argtypes = [C.c_char_p]
        L.xpbd_multi_config_default.argtypes = [C.POINTER(MultiConfig)]
        L.xpbd_multi_config_default.restype = None
        L.xpbd_multi_world_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(MultiConfig)]
        L.xpbd_multi_world_destroy.argtypes = [C.c_void_p]
        L.xpbd_multi_world_destroy.restype = None
        L.xpbd_multi_world_set_polytopes.argtypes = [C.c_void_p, C.POINTER(PolytopeDesc), C.c_uint32]
        L.xpbd_multi_world_upload.argtypes = [C.c_void_p, C.c_void_p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        L.xpbd_multi_world_step.argtypes = [C.c_void_p, C.c_double, C.c_uint32]
        L.xpbd_multi_world_replan.argtypes = [C.c_void_p]
        L.xpbd_multi_world_synchronize.argtypes = [C.c_void_p]
        L.xpbd_multi_world_download.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_multi_world_halo_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), _f64p]
        L.xpbd_multi_world_contact_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        try:
            L.xpbd_multi_world_download_owned.argtypes = [C.c_void_p, _u32p, C.c_void_p, C.c_uint32, _u32p]
            L.xpbd_multi_world_plan_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            L.xpbd_multi_world_owners.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB for an A/B measurement (scripts/)
            pass
        L.xpbd_halo_cell_key.argtypes = [_f64p, C.c_double]
        L.xpbd_halo_cell_key.restype = C.c_int64
        L.xpbd_halo_plan.argtypes = [C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p, _u32p,
                                     _u32p, C.c_uint32]
        L.xpbd_world_set_polytopes.argtypes = [C.c_void_p, C.POINTER(PolytopeDesc), C.c_uint32]
        L.xpbd_world_narrowphase.argtypes = [C.c_void_p, _u32p, C.c_uint32, C.c_void_p]
        L.xpbd_world_edge_axes_separation.argtypes = [C.c_void_p, _u32p, C.c_uint32, C.c_void_p]
        L.xpbd_world_narrowphase_gjk.argtypes = [C.c_void_p, _u32p, C.c_uint32, C.c_void_p]
        L.xpbd_world_set_narrowphase.argtypes = [C.c_void_p, C.c_uint32]
        L.xpbd_world_set_contact_pad.argtypes = [C.c_void_p, C.c_double]
        try:
            L.xpbd_world_set_max_depenetration_speed.argtypes = [C.c_void_p, C.c_double]
            L.xpbd_multi_world_set_max_depenetration_speed.argtypes = [C.c_void_p, C.c_double]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        L.xpbd_world_contact_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.xpbd_world_build_neighbours.argtypes = [C.c_void_p, C.c_double, _u32p]
        L.xpbd_world_download_neighbours.argtypes = [C.c_void_p, _u32p, _u32p, C.c_uint32]
        L.xpbd_world_set_joints.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_world_set_joint_limits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_multi_world_set_joint_limits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_world_set_joint_drives.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_multi_world_set_joint_drives.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.xpbd_world_contacts_begin.argtypes = [C.c_void_p, C.c_double]
        L.xpbd_world_contacts_substep.argtypes = [C.c_void_p, C.c_double]
        L.xpbd_world_export_dynamic.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.xpbd_world_import_dynamic.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.xpbd_world_import_dynamic_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.xpbd_world_set_sat_schedule.argtypes = [C.c_void_p, C.c_uint32]
        L.xpbd_world_history_push.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.xpbd_world_history_restore.argtypes = [C.c_void_p, C.c_uint32]
        L.xpbd_world_history_truncate.argtypes = [C.c_void_p, C.c_uint32]
        L.xpbd_world_history_length.argtypes = [C.c_void_p]
        L.xpbd_world_history_length.restype = C.c_uint32
        L.xpbd_world_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.xpbd_world_raycast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.xpbd_multi_world_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        try:
            L.xpbd_world_set_collision_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            L.xpbd_multi_world_set_collision_filters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            L.xpbd_world_raycast_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_raycast_masked_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_multi_world_raycast_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_contact_report.argtypes = [C.c_void_p, C.c_uint32]
            L.xpbd_world_contact_report_counts.argtypes = [C.c_void_p, _u32p]
            L.xpbd_world_download_pair_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p]
            L.xpbd_world_download_contact_events.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
            L.xpbd_multi_world_set_contact_report.argtypes = [C.c_void_p, C.c_uint32]
            L.xpbd_multi_world_contact_report_counts.argtypes = [C.c_void_p, _u32p]
            L.xpbd_multi_world_download_pair_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p]
            L.xpbd_multi_world_download_contact_events.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double]
            L.xpbd_multi_world_set_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_restitution.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_external_wrench.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.xpbd_world_set_external_wrench_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.xpbd_world_apply_impulses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_apply_impulses_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_dynamics.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.xpbd_world_get_dynamics.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.xpbd_multi_world_set_external_wrench.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.xpbd_multi_world_apply_impulses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            ovl = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_overlap.argtypes = ovl + [_u32p]
            L.xpbd_world_overlap_device.argtypes = ovl
            L.xpbd_multi_world_overlap.argtypes = ovl + [_u32p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_sweep_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_multi_world_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_distance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_multi_world_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_terrain_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.xpbd_world_terrain_distance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_remove_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, _u32p]
            L.xpbd_world_remove_bodies_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u32p]
            L.xpbd_world_add_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_terrain.argtypes = [C.c_void_p, C.POINTER(HEIGHTFIELD)]
            L.xpbd_world_sample_terrain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_islands.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, _u32p]
            L.xpbd_world_islands_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_sleeping.argtypes = [C.c_void_p, C.POINTER(SLEEP_CONFIG)]
            L.xpbd_world_sleep_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u32p]
            L.xpbd_world_sleep_state_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.xpbd_world_wake_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_wake_bodies_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_joint_states.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.xpbd_world_joint_states_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.xpbd_world_set_drive_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_drive_targets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_damping.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_get_damping.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_joint_damping.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_kinematics.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_kinematic_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_kinematic_targets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_kinematic_count.argtypes = [C.c_void_p]
            L.xpbd_world_kinematic_count.restype = C.c_uint32
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_mass_properties.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
            L.xpbd_world_set_mass_properties_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
            L.xpbd_world_get_mass_properties.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        try:
            L.xpbd_world_set_sensors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_get_sensors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            L.xpbd_world_sensor_count.argtypes = [C.c_void_p]
            L.xpbd_world_sensor_count.restype = C.c_uint32
            L.xpbd_world_sensor_overlaps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.xpbd_world_sensor_overlaps_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        except AttributeError:          # an older build loaded through XPBD_HIP_LIB
            pass
        _hip = L
    return _hip


def host_lib():
    global _host
    if _host is None:
        hip_lib()  # libxpbd_host.so links against it
        L = _load("libxpbd_host.so")
        L.xpbdh_scene_shapes.argtypes = [C.c_uint32, _f64p, C.c_uint32, _u32p, C.c_uint32]
        L.xpbdh_scene_generate.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p]
        L.xpbdh_default_grid_width.argtypes = [C.c_uint32]
        L.xpbdh_default_grid_width.restype = C.c_uint32
        L.xpbdh_rigid_metrics.argtypes = [C.c_uint32, C.c_double, C.c_double, _f64p]
        L.xpbdh_rigid_metrics.restype = None
        L.xpbdh_rigid_new.argtypes = [_f64p, C.c_void_p]
        L.xpbdh_rigid_frame.argtypes = [C.c_void_p, _f64p]
        L.xpbdh_rigid_frame.restype = None
        L.xpbdh_world_new.argtypes = [C.c_void_p, C.c_void_p]
        L.xpbdh_shape_plane.argtypes = [C.c_uint32, C.c_double, C.c_uint32, _f64p]
        L.xpbdh_polytope_arrays.argtypes = [C.c_uint32, C.c_double, _u32p, _f64p, _u32p, _u32p, _u32p, _f64p]
        L.xpbdh_polytope_arrays.restype = None
        _host = L
    return _host


def _check(rc):
    if rc != OK:
        raise XpbdError(rc, hip_lib().xpbd_last_error().decode())


def _f64(a):
    return a.ctypes.data_as(_f64p)


def _u32(a):
    return a.ctypes.data_as(_u32p)


class World:
    """N-body world on one GPU: thin wrapper over xpbd_world_* (reference World::integrate, src/world.rs:34-43)."""

    def __init__(self, device=0, mode=MODE_FUSED, trace_contacts=False, block_size=0):
        L = hip_lib()
        cfg = Config()
        L.xpbd_config_default(C.byref(cfg))
        cfg.device, cfg.mode, cfg.block_size = device, mode, block_size
        cfg.flags = FLAG_TRACE_CONTACTS if trace_contacts else 0
        self._h = C.c_void_p()
        _check(L.xpbd_world_create(C.byref(self._h), C.byref(cfg)))
        self.n = 0
        self.n_joints = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            hip_lib().xpbd_world_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_shapes(self, verts_xyz, vert_offsets):
        v = np.ascontiguousarray(verts_xyz, dtype=np.float64).reshape(-1)
        o = np.ascontiguousarray(vert_offsets, dtype=np.uint32)
        if v.size == 0:
            v = np.zeros(3)
        _check(hip_lib().xpbd_world_set_shapes(self._h, _f64(v), _u32(o), o.size - 1))

    def upload(self, bodies, shape_id=None):
        b = np.ascontiguousarray(bodies, dtype=np.float64).reshape(-1, RIGID_DOUBLES)
        sid = None if shape_id is None else np.ascontiguousarray(shape_id, dtype=np.uint32)
        _check(hip_lib().xpbd_world_upload_bodies(self._h, b.ctypes.data, None if sid is None else _u32(sid), b.shape[0]))
        self.n = b.shape[0]
        self.n_joints = 0

    def step(self, dt, substeps):
        _check(hip_lib().xpbd_world_step(self._h, dt, substeps))

    def synchronize(self):
        _check(hip_lib().xpbd_world_synchronize(self._h))

    def download(self):
        out = np.empty((self.n, RIGID_DOUBLES), dtype=np.float64)
        _check(hip_lib().xpbd_world_download_bodies(self._h, out.ctypes.data, self.n))
        return out

    def frames(self):
        """(n, 7) Rigid::frame() of every body: origin xyz, rotation sxyz (what the reference's renderer reads)."""
        out = np.empty((self.n, 7), dtype=np.float64)
        _check(hip_lib().xpbd_world_download_frames(self._h, _f64(out), self.n))
        return out

    def contacts(self):
        """(k, 2) uint32 array of (body, vertex) of the last substep, reference push order."""
        n = C.c_uint32(0)
        rc = hip_lib().xpbd_world_download_contacts(self._h, None, 0, C.byref(n))
        if rc not in (OK, E_CAPACITY):
            _check(rc)
        out = np.empty((n.value, 2), dtype=np.uint32)
        if n.value:
            _check(hip_lib().xpbd_world_download_contacts(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def contact_masks(self, substeps):
        out = np.empty((substeps, self.n), dtype=np.uint32)
        _check(hip_lib().xpbd_world_download_contact_masks(self._h, _u32(out), substeps, self.n))
        return out

    def set_polytopes(self, polytopes):
        """polytopes: list of dicts with vertices (V,3), edges (E,2), face_offsets (F+1), face_indices, centroid (3)."""
        descs, _keep = polytope_descs(polytopes)
        _check(hip_lib().xpbd_world_set_polytopes(self._h, descs, len(polytopes)))

    def narrowphase(self, pairs):
        """SAT manifolds (MANIFOLD_DTYPE records) of the given (A, B) body pairs at the current poses."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(pr.shape[0], dtype=MANIFOLD_DTYPE)
        _check(hip_lib().xpbd_world_narrowphase(self._h, _u32(pr), pr.shape[0], out.ctypes.data))
        return out

    def edge_axes_separation(self, pairs):
        """The reference's edge_axes_separation (src/collision.rs:151-197) of the given (A, B) pairs: EDGE_QUERY_DTYPE records."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(pr.shape[0], dtype=EDGE_QUERY_DTYPE)
        _check(hip_lib().xpbd_world_edge_axes_separation(self._h, _u32(pr), pr.shape[0], out.ctypes.data))
        return out

    def narrowphase_gjk(self, pairs):
        """GJK + EPA results (GJK_DTYPE records) of the given (A, B) body pairs at the current poses."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(pr.shape[0], dtype=GJK_DTYPE)
        _check(hip_lib().xpbd_world_narrowphase_gjk(self._h, _u32(pr), pr.shape[0], out.ctypes.data))
        return out

    def set_narrowphase(self, narrowphase):
        _check(hip_lib().xpbd_world_set_narrowphase(self._h, narrowphase))

    def set_contact_pad(self, pad):
        _check(hip_lib().xpbd_world_set_contact_pad(self._h, pad))

    def set_max_depenetration_speed(self, speed):
        """Limit on how fast a body-body contact may push its bodies apart (m/s); 0 = off = the reference's solver loop."""
        _check(hip_lib().xpbd_world_set_max_depenetration_speed(self._h, speed))

    def contact_stats(self):
        """(neighbour pairs of the last step, touching pairs, manifold points) -- the last two since the previous call."""
        out = (C.c_uint64 * 3)()
        _check(hip_lib().xpbd_world_contact_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def neighbours(self, dt):
        """Runs the sphere broadphase as step(dt, .) would: (offsets[n+1], neighbours) CSR, ascending."""
        n_entries = C.c_uint32(0)
        _check(hip_lib().xpbd_world_build_neighbours(self._h, dt, C.byref(n_entries)))
        off = np.zeros(self.n + 1, dtype=np.uint32)
        nb = np.zeros(max(n_entries.value, 1), dtype=np.uint32)
        _check(hip_lib().xpbd_world_download_neighbours(self._h, _u32(off), _u32(nb), nb.size))
        return off, nb[: n_entries.value]

    def set_joints(self, joints):
        """joints: JOINT_DTYPE records naming bodies of the last upload (extension; XPBD_MODE_CONTACTS)."""
        j = np.ascontiguousarray(joints, dtype=JOINT_DTYPE)
        _check(hip_lib().xpbd_world_set_joints(self._h, j.ctypes.data if j.size else None, j.size))
        self.n_joints = j.size

    def set_joint_limits(self, limits):
        """limits: JOINT_LIMIT_DTYPE records naming joints of the last set_joints (extension; empty clears them)."""
        lim = np.ascontiguousarray(limits, dtype=JOINT_LIMIT_DTYPE)
        _check(hip_lib().xpbd_world_set_joint_limits(self._h, lim.ctypes.data if lim.size else None, lim.size))

    def set_joint_drives(self, drives):
        """drives: JOINT_DRIVE_DTYPE records naming joints of the last set_joints (extension; empty clears them)."""
        drv = np.ascontiguousarray(drives, dtype=JOINT_DRIVE_DTYPE)
        _check(hip_lib().xpbd_world_set_joint_drives(self._h, drv.ctypes.data if drv.size else None, drv.size))

    def set_collision_filters(self, filters=None, flags=0):
        """filters: COLLISION_FILTER_DTYPE records, one per body of the last upload, or None for the default {~0, ~0}
        (extension); flags: FILTER_JOINTED or 0."""
        f = _filters(filters)
        _check(hip_lib().xpbd_world_set_collision_filters(self._h, None if f is None else f.ctypes.data, 0 if f is None else f.size, flags))

    def set_materials(self, materials=None, ground_friction=np.inf):
        """materials: MATERIAL_DTYPE records or plain friction coefficients, one per body of the last upload, or None for
        the default +inf (extension; XPBD_MODE_CONTACTS); ground_friction: the coefficient of the plane z = 0."""
        m = _materials(materials)
        _check(hip_lib().xpbd_world_set_materials(self._h, None if m is None else m.ctypes.data, 0 if m is None else m.size, ground_friction))

    def set_restitution(self, restitution=None, ground_restitution=0.0, bounce_threshold=0.0):
        """restitution: coefficients in [0, 1], one per body of the last upload, or None for the default 0 (extension;
        XPBD_MODE_CONTACTS); ground_restitution: the coefficient of the plane z = 0; bounce_threshold: closing speed (m/s) below
        which a contact does not bounce."""
        e = None if restitution is None else np.ascontiguousarray(restitution, dtype=np.float64).reshape(-1)
        _check(hip_lib().xpbd_world_set_restitution(self._h, None if e is None else e.ctypes.data, 0 if e is None else e.size,
                                                    ground_restitution, bounce_threshold))

    def set_damping(self, rows=None):
        """rows: BODY_DAMPING_DTYPE records (see body_damping()), one per body, or None for the default row everywhere (extension;
        XPBD_MODE_CONTACTS; include/xpbd.h, "DAMPING")."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=BODY_DAMPING_DTYPE).reshape(-1)
        _check(hip_lib().xpbd_world_set_damping(self._h, None if r is None else r.ctypes.data, 0 if r is None else r.size))

    def get_damping(self):
        """The rows in force, one BODY_DAMPING_DTYPE record per body."""
        rows = np.zeros(self.n, dtype=BODY_DAMPING_DTYPE)
        _check(hip_lib().xpbd_world_get_damping(self._h, rows.ctypes.data if rows.size else None, rows.size))
        return rows

    def set_joint_damping(self, dampers=None):
        """Replaces the joint dampers: JOINT_DAMPING_DTYPE records (see joint_damping()), at most one per joint of the last
        set_joints; None or an empty list clears them."""
        d = np.zeros(0, dtype=JOINT_DAMPING_DTYPE) if dampers is None else np.ascontiguousarray(dampers, dtype=JOINT_DAMPING_DTYPE).reshape(-1)
        _check(hip_lib().xpbd_world_set_joint_damping(self._h, d.ctypes.data if d.size else None, d.size))

    def set_terrain(self, heights=None, origin=(0.0, 0.0), cell=(1.0, 1.0)):
        """heights: (ny, nx) array, heights[iy, ix] at world (origin[0] + ix * cell[0], origin[1] + iy * cell[1]), the ground
        of XPBD_MODE_CONTACTS in place of the plane z = 0 (extension); None: back to the plane."""
        if heights is None:
            _check(hip_lib().xpbd_world_set_terrain(self._h, None))
            return
        h = np.ascontiguousarray(heights, dtype=np.float64)
        if h.ndim != 2:
            raise ValueError("heights must be a 2-d array (ny rows of nx)")
        hf = HEIGHTFIELD(h.shape[1], h.shape[0], (C.c_double * 2)(*origin), (C.c_double * 2)(*cell), _f64(h))
        _check(hip_lib().xpbd_world_set_terrain(self._h, C.byref(hf)))

    def sample_terrain(self, xy, normals=True):
        """(height[n], normal[n, 3]) of the terrain under the points xy (n, 2): NaN and (0, 0, 0) outside the field.
        normals=False: the heights alone."""
        p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        height = np.empty(p.shape[0], dtype=np.float64)
        normal = np.empty((p.shape[0], 3), dtype=np.float64) if normals else None
        _check(hip_lib().xpbd_world_sample_terrain(self._h, p.ctypes.data, p.shape[0], height.ctypes.data,
                                                   None if normal is None else normal.ctypes.data))
        return (height, normal) if normals else height

    def contacts_begin(self, dt):
        _check(hip_lib().xpbd_world_contacts_begin(self._h, dt))

    def contacts_substep(self, h):
        _check(hip_lib().xpbd_world_contacts_substep(self._h, h))

    def export_dynamic(self, dev_indices_ptr, n, dev_buf_ptr):
        """Device pointers (e.g. torch tensor .data_ptr()): n uint32 indices, n x 13 doubles."""
        _check(hip_lib().xpbd_world_export_dynamic(self._h, C.c_void_p(dev_indices_ptr), n, C.c_void_p(dev_buf_ptr)))

    def import_dynamic(self, dev_indices_ptr, n, dev_buf_ptr):
        _check(hip_lib().xpbd_world_import_dynamic(self._h, C.c_void_p(dev_indices_ptr), n, C.c_void_p(dev_buf_ptr)))

    def import_dynamic_rows(self, dev_indices_ptr, dev_rows_ptr, n, dev_buf_ptr):
        """Body indices[k] takes row rows[k] of the buffer (device pointers; rows are uint32)."""
        _check(hip_lib().xpbd_world_import_dynamic_rows(self._h, C.c_void_p(dev_indices_ptr), C.c_void_p(dev_rows_ptr), n,
                                                        C.c_void_p(dev_buf_ptr)))

    def set_sat_schedule(self, schedule):
        """SAT_SCHEDULE_AUTO / _ONE_PASS / _TWO_PASS (same results, different cost)."""
        _check(hip_lib().xpbd_world_set_sat_schedule(self._h, schedule))

    # state history: the reference app's `states` vector and `current_state` cursor (src/app.rs:48, 206-212)
    def history_push(self):
        index = C.c_uint32(0)
        _check(hip_lib().xpbd_world_history_push(self._h, C.byref(index)))
        return index.value

    def history_restore(self, index):
        _check(hip_lib().xpbd_world_history_restore(self._h, index))

    def history_truncate(self, length):
        _check(hip_lib().xpbd_world_history_truncate(self._h, length))

    def history_length(self):
        return hip_lib().xpbd_world_history_length(self._h)

    def raycast(self, rays, flags=0, mask=None):
        """RAY_HIT_DTYPE records of the closest body along every ray (RAY_DTYPE records, see rays()) at the current poses.
        mask: only bodies whose collision-filter group meets it can be hit (None: every body).
        flags | QUERY_TERRAIN: the terrain stops rays too (body = HIT_TERRAIN, face = the triangle, or RAY_INSIDE from in or
        under the ground); it needs set_terrain, and neither mask nor ignore_body concerns it."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        out = np.zeros(r.size, dtype=RAY_HIT_DTYPE)
        rp, hp = r.ctypes.data if r.size else None, out.ctypes.data if r.size else None
        if mask is None:
            _check(hip_lib().xpbd_world_raycast(self._h, rp, r.size, flags, hp))
        else:
            _check(hip_lib().xpbd_world_raycast_masked(self._h, rp, r.size, flags, mask, hp))
        return out

    def raycast_device(self, rays_ptr, n, hits_ptr, flags=0, mask=None):
        """Device arrays of n xpbd_ray / xpbd_ray_hit, stream-ordered on the world's stream."""
        if mask is None:
            _check(hip_lib().xpbd_world_raycast_device(self._h, C.c_void_p(rays_ptr), n, flags, C.c_void_p(hits_ptr)))
        else:
            _check(hip_lib().xpbd_world_raycast_masked_device(self._h, C.c_void_p(rays_ptr), n, flags, mask, C.c_void_p(hits_ptr)))

    def overlap(self, queries, flags=0):
        """(offsets, hits) of the bodies every convex volume touches (OVERLAP_QUERY_DTYPE records, see overlap_queries()) at the
        current poses: the hits of query q are hits[offsets[q]:offsets[q + 1]] (OVERLAP_HIT_DTYPE), in ascending body index.
        flags | QUERY_TERRAIN: a volume with a vertex under the ground (the stepper's ground contact) gets one more entry, the
        last of its segment: {HIT_TERRAIN, FEATURE_FACE_B, the deepest vertex's signed distance}."""
        return _overlap(hip_lib().xpbd_world_overlap, self._h, queries, flags)

    def overlap_device(self, queries_ptr, n, offsets_ptr, hits_ptr, cap, flags=0):
        """Device arrays of n xpbd_overlap_query, n + 1 uint32 offsets and cap xpbd_overlap_hit, stream-ordered on the world's
        stream; the total is offsets[n], hits beyond cap are not written."""
        _check(hip_lib().xpbd_world_overlap_device(self._h, C.c_void_p(queries_ptr), n, flags, C.c_void_p(offsets_ptr),
                                                   C.c_void_p(hits_ptr) if hits_ptr else None, cap))

    def sweep(self, sweeps, flags=0):
        """SWEEP_HIT_DTYPE records of the first body every convex volume hits when moved along its segment (SWEEP_DTYPE records,
        see sweeps()) at the current poses.
        flags | QUERY_TERRAIN: the volume also stops where its first vertex goes under the ground (body = HIT_TERRAIN, feature =
        FEATURE_FACE_B, face = the triangle; SWEEP_INITIAL when a vertex starts there), if that is strictly earlier."""
        return _sweep(hip_lib().xpbd_world_sweep, self._h, sweeps, flags)

    def sweep_device(self, sweeps_ptr, n, hits_ptr, flags=0):
        """Device arrays of n xpbd_sweep and n xpbd_sweep_hit, stream-ordered on the world's stream."""
        _check(hip_lib().xpbd_world_sweep_device(self._h, C.c_void_p(sweeps_ptr), n, flags, C.c_void_p(hits_ptr)))

    def distance(self, queries, flags=0):
        """DISTANCE_HIT_DTYPE records of the body nearest to every convex volume or point (DISTANCE_QUERY_DTYPE records, see
        distances()) at the current poses: the distance, the two closest points and the normal from the body to the volume;
        DISTANCE_OVERLAP at distance 0 where the overlap query would list the body."""
        return _distance(hip_lib().xpbd_world_distance, self._h, queries, flags)

    def distance_device(self, queries_ptr, n, hits_ptr, flags=0):
        """Device arrays of n xpbd_distance_query and n xpbd_distance_hit, stream-ordered on the world's stream."""
        _check(hip_lib().xpbd_world_distance_device(self._h, C.c_void_p(queries_ptr), n, flags, C.c_void_p(hits_ptr)))

    def terrain_distance(self, queries, flags=0):
        """DISTANCE_HIT_DTYPE records of the feature of the TERRAIN's surface nearest to every convex volume or point
        (DISTANCE_QUERY_DTYPE records, see distances(); ignore_body and mask are not read): body HIT_TERRAIN, the distance, the
        two closest points and the normal from the ground to the volume; DISTANCE_OVERLAP at distance 0 where a vertex is under
        the ground or a terrain edge enters the volume.  index_b numbers the triangle (FACE_B), sample (FACE_A) or terrain edge
        (EDGES).  The world's nearest thing is the smaller distance of this and distance(); a body wins a tie."""
        return _distance(hip_lib().xpbd_world_terrain_distance, self._h, queries, flags)

    def terrain_distance_device(self, queries_ptr, n, hits_ptr, flags=0):
        """Device arrays of n xpbd_distance_query and n xpbd_distance_hit, stream-ordered on the world's stream; never waits."""
        _check(hip_lib().xpbd_world_terrain_distance_device(self._h, C.c_void_p(queries_ptr), n, flags, C.c_void_p(hits_ptr)))

    # body edits (include/xpbd.h, "Body EDITS"): forces, impulses and state of resident bodies
    def set_external_wrench(self, indices=None, force=None, torque=None):
        """external_force / external_torque of the listed bodies (None: all bodies, in order) = rows of force / torque
        ((n, 3); None leaves that field alone).  Waits."""
        _check(_set_wrench(hip_lib().xpbd_world_set_external_wrench, self._h, indices, force, torque))

    def set_external_wrench_device(self, dev_indices_ptr, n, dev_force_ptr, dev_torque_ptr):
        """Device pointers (0 / None: no index list, a field left alone), stream-ordered on the world's stream."""
        _check(hip_lib().xpbd_world_set_external_wrench_device(self._h, C.c_void_p(dev_indices_ptr or None), n,
                                                               C.c_void_p(dev_force_ptr or None), C.c_void_p(dev_torque_ptr or None)))

    def apply_impulses(self, impulses):
        """impulses: IMPULSE_DTYPE records (see impulses()), applied per body in list order.  Waits."""
        imp = np.ascontiguousarray(impulses, dtype=IMPULSE_DTYPE).reshape(-1)
        _check(hip_lib().xpbd_world_apply_impulses(self._h, imp.ctypes.data if imp.size else None, imp.size))

    def apply_impulses_device(self, dev_list_ptr, n):
        """Device array of n xpbd_impulse, the entries of one body adjacent; stream-ordered on the world's stream."""
        _check(hip_lib().xpbd_world_apply_impulses_device(self._h, C.c_void_p(dev_list_ptr), n))

    def set_dynamics(self, indices, rows):
        """rows: (n, 13) position, rotation {s,x,y,z}, velocity, angular_velocity of the listed bodies (None: all).  Waits."""
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, DYNAMIC_DOUBLES)
        _check(hip_lib().xpbd_world_set_dynamics(self._h, None if idx is None else idx.ctypes.data, r.shape[0], r.ctypes.data if r.size else None))

    def get_dynamics(self, indices=None):
        """(n, 13) rows of the listed bodies (None: all bodies, in order)."""
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        n = self.n if idx is None else idx.size
        out = np.empty((n, DYNAMIC_DOUBLES), dtype=np.float64)
        _check(hip_lib().xpbd_world_get_dynamics(self._h, None if idx is None else idx.ctypes.data, n, out.ctypes.data if n else None))
        return out

    # mass edits (include/xpbd.h, "MASS properties of resident bodies"): freeze, release, re-weigh
    def set_mass_properties(self, indices, rows, flags=MASS_INVERSE):
        """rows: (n, 13) of the listed bodies (None: all) in the layout flags names -- MASS_INVERSE: inverse_mass,
        inverse_inertia[9], center_of_mass[3]; MASS_DIRECT: mass, inertia[9], center_of_mass[3], inverted on the device; with
        MASS_KEEP_FRAME the geometry stays where it is when the centre of mass changes.  Waits."""
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, MASS_DOUBLES)
        _check(hip_lib().xpbd_world_set_mass_properties(self._h, None if idx is None else idx.ctypes.data, r.shape[0],
                                                        r.ctypes.data if r.size else None, flags))

    def set_mass_properties_device(self, dev_indices_ptr, n, dev_rows_ptr, flags=MASS_INVERSE):
        """Device pointers (0 / None: no index list), stream-ordered on the world's stream; an invalid entry is skipped."""
        _check(hip_lib().xpbd_world_set_mass_properties_device(self._h, C.c_void_p(dev_indices_ptr or None), n, C.c_void_p(dev_rows_ptr or None), flags))

    def get_mass_properties(self, indices=None):
        """(n, 13) rows of the listed bodies (None: all bodies, in order), always in the MASS_INVERSE layout."""
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        n = self.n if idx is None else idx.size
        out = np.empty((n, MASS_DOUBLES), dtype=np.float64)
        _check(hip_lib().xpbd_world_get_mass_properties(self._h, None if idx is None else idx.ctypes.data, n, out.ctypes.data if n else None))
        return out

    # body population (include/xpbd.h, "Body POPULATION"): removing resident bodies and appending new ones
    def remove_bodies(self, indices):
        """Removes the listed bodies (an index may be listed twice); the survivors keep their order and their settings.
        Returns (old_to_new, joint_old_to_new): uint32 arrays of the old body and joint counts, NO_HIT for what is gone.  Waits."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        old_to_new = np.empty(self.n, dtype=np.uint32)
        joint_old_to_new = np.empty(self.n_joints, dtype=np.uint32)
        n_out = C.c_uint32(self.n)
        _check(hip_lib().xpbd_world_remove_bodies(self._h, idx.ctypes.data if idx.size else None, idx.size,
                                                  old_to_new.ctypes.data if self.n else None,
                                                  joint_old_to_new.ctypes.data if self.n_joints else None, C.byref(n_out)))
        self.n = n_out.value
        self.n_joints = int(np.count_nonzero(joint_old_to_new != NO_HIT))
        return old_to_new, joint_old_to_new

    def remove_bodies_device(self, dev_ptr, dev_map_ptr=None):
        """dev_ptr: device array of one byte per body, nonzero = remove, produced on the world's stream or ordered before it;
        dev_map_ptr: device uint32 array of the old body count that receives old_to_new, or None.  Returns joint_old_to_new.  Waits."""
        joint_old_to_new = np.empty(self.n_joints, dtype=np.uint32)
        n_out = C.c_uint32(self.n)
        _check(hip_lib().xpbd_world_remove_bodies_device(self._h, C.c_void_p(dev_ptr or None), C.c_void_p(dev_map_ptr or None),
                                                         joint_old_to_new.ctypes.data if self.n_joints else None, C.byref(n_out)))
        self.n = n_out.value
        self.n_joints = int(np.count_nonzero(joint_old_to_new != NO_HIT))
        return joint_old_to_new

    def add_bodies(self, bodies, shape_id):
        """Appends bodies ((k, 38) rows with their shape ids) with the default settings; returns the index of the first.  Waits."""
        b = np.ascontiguousarray(bodies, dtype=np.float64).reshape(-1, RIGID_DOUBLES)
        sid = np.ascontiguousarray(shape_id, dtype=np.uint32).reshape(-1)
        if sid.size != b.shape[0]:
            raise ValueError("add_bodies: %d bodies but %d shape ids" % (b.shape[0], sid.size))
        first = C.c_uint32(self.n)
        _check(hip_lib().xpbd_world_add_bodies(self._h, b.ctypes.data if b.size else None, sid.ctypes.data if sid.size else None,
                                               b.shape[0], C.byref(first)))
        self.n += b.shape[0]
        return first.value

    def get_stream(self):
        return hip_lib().xpbd_world_get_stream(self._h)

    def set_stream(self, stream_ptr):
        _check(hip_lib().xpbd_world_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_mode(self, mode):
        _check(hip_lib().xpbd_world_set_mode(self._h, mode))

    # contact reports (include/xpbd.h, "Contact REPORTS"): the touching pairs of the current frame, their last manifolds and the
    # begin / end events against the previous frame
    def set_contact_report(self, enable):
        _check(hip_lib().xpbd_world_set_contact_report(self._h, 1 if enable else 0))

    def contact_report_counts(self):
        """(pairs, points, begins, ends) of the current frame's report."""
        return _report_counts(hip_lib().xpbd_world_contact_report_counts, self._h)

    def pair_contacts(self, points=True):
        """(PAIR_CONTACT_DTYPE records, CONTACT_POINT_DTYPE records or None) of the current frame."""
        return _pair_contacts(hip_lib().xpbd_world_contact_report_counts, hip_lib().xpbd_world_download_pair_contacts, self._h, points)

    def contact_events(self):
        """CONTACT_EVENT_DTYPE records: BEGINs then ENDs, each in (body_a, body_b) order."""
        return _contact_events(hip_lib().xpbd_world_contact_report_counts, hip_lib().xpbd_world_download_contact_events, self._h)

    # contact islands (include/xpbd.h, "Contact ISLANDS"): connected groups of the non-fixed bodies and their rest state
    def islands(self, flags=0, cap=None):
        """(island_of, ISLAND_DTYPE records): island_of[i] = island of body i, ISLAND_NONE for a fixed body.  cap: room for
        that many records (None: one per body, which always suffices; a smaller one raises E_CAPACITY when it is short).  Waits."""
        island_of = np.empty(self.n, dtype=np.uint32)
        room = self.n if cap is None else cap
        out = np.zeros(room, dtype=ISLAND_DTYPE)
        total = C.c_uint32(0)
        _check(hip_lib().xpbd_world_islands(self._h, flags, island_of.ctypes.data if self.n else None, out.ctypes.data if room else None,
                                            room, C.byref(total)))
        return island_of, out[:total.value]

    def islands_device(self, flags, dev_island_of_ptr, dev_islands_ptr, cap, dev_n_islands_ptr):
        """Device arrays (island_of: uint32 per body or None; records: cap x 40 bytes, 8-byte aligned; the count: one uint32);
        enqueues on the world's stream and returns at once."""
        _check(hip_lib().xpbd_world_islands_device(self._h, flags, C.c_void_p(dev_island_of_ptr or None), C.c_void_p(dev_islands_ptr or None),
                                                   cap, C.c_void_p(dev_n_islands_ptr or None)))

    # island sleeping (include/xpbd.h, "SLEEPING"): resting islands leave the step until something disturbs them
    def set_sleeping(self, linear_speed=None, angular_speed=None, frames_to_sleep=None, flags=0):
        """Turns sleeping on with these thresholds, or off when called without arguments."""
        if linear_speed is None and angular_speed is None and frames_to_sleep is None:
            _check(hip_lib().xpbd_world_set_sleeping(self._h, None))
            return
        cfg = SLEEP_CONFIG(linear_speed, angular_speed, frames_to_sleep, flags)
        _check(hip_lib().xpbd_world_set_sleeping(self._h, C.byref(cfg)))

    def sleep_state(self):
        """(asleep uint8[n], rest_frames uint32[n], group uint32[n], (asleep bodies, sleeping groups, woken, put to sleep by the
        last pass)).  Waits."""
        asleep = np.zeros(self.n, dtype=np.uint8)
        rest = np.zeros(self.n, dtype=np.uint32)
        group = np.zeros(self.n, dtype=np.uint32)
        counts = (C.c_uint32 * 4)()
        _check(hip_lib().xpbd_world_sleep_state(self._h, asleep.ctypes.data if self.n else None, rest.ctypes.data if self.n else None,
                                                group.ctypes.data if self.n else None, counts))
        return asleep, rest, group, tuple(int(v) for v in counts)

    def sleep_state_device(self, dev_asleep_ptr, dev_rest_frames_ptr, dev_group_ptr, dev_counts_ptr):
        """Device arrays (any may be None); enqueues on the world's stream and returns at once."""
        _check(hip_lib().xpbd_world_sleep_state_device(self._h, C.c_void_p(dev_asleep_ptr or None), C.c_void_p(dev_rest_frames_ptr or None),
                                                       C.c_void_p(dev_group_ptr or None), C.c_void_p(dev_counts_ptr or None)))

    def wake_bodies(self, indices=None):
        """The groups of the listed bodies wake at the start of the next step; None: everybody."""
        if indices is None:
            _check(hip_lib().xpbd_world_wake_bodies(self._h, None, 0))
            return
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        _check(hip_lib().xpbd_world_wake_bodies(self._h, idx.ctypes.data if idx.size else None, idx.size))

    def wake_bodies_device(self, dev_indices_ptr, n):
        _check(hip_lib().xpbd_world_wake_bodies_device(self._h, C.c_void_p(dev_indices_ptr or None), n))

    # joint states and drive targets (include/xpbd.h, "Joint STATES and drive TARGETS")
    def joint_states(self, joints=None):
        """JOINT_STATE_DTYPE records of the listed joints; None: all of them.  Reads only; waits."""
        if joints is None:
            n = self.n_joints
            out = np.zeros(n, dtype=JOINT_STATE_DTYPE)
            _check(hip_lib().xpbd_world_joint_states(self._h, None, n, out.ctypes.data if n else None))
            return out
        idx = np.ascontiguousarray(joints, dtype=np.uint32)
        out = np.zeros(idx.size, dtype=JOINT_STATE_DTYPE)
        if idx.size:
            _check(hip_lib().xpbd_world_joint_states(self._h, idx.ctypes.data, idx.size, out.ctypes.data))
        return out

    def joint_states_device(self, dev_joints_ptr, n, dev_out_ptr):
        """Device arrays (joints: uint32 or None for joints 0..n-1; out: n x 80 bytes, 16-byte aligned); enqueues on the world's
        stream and returns at once.  An index out of range gives a record with kind = JOINT_STATE_NO_JOINT."""
        _check(hip_lib().xpbd_world_joint_states_device(self._h, C.c_void_p(dev_joints_ptr or None), n, C.c_void_p(dev_out_ptr or None)))

    def set_drive_targets(self, drives, targets):
        """Replaces the targets of the listed drives of the last set_joint_drives (strictly ascending indices; None: all of
        them, one target each) and nothing else of them.  Waits."""
        tgt = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1)
        idx = None if drives is None else np.ascontiguousarray(drives, dtype=np.uint32)
        if idx is not None and idx.size != tgt.size:
            raise ValueError("set_drive_targets: %d drives but %d targets" % (idx.size, tgt.size))
        if idx is not None and idx.size == 0:
            return
        _check(hip_lib().xpbd_world_set_drive_targets(self._h, None if idx is None else idx.ctypes.data, tgt.ctypes.data if tgt.size else None, tgt.size))

    def set_drive_targets_device(self, dev_drives_ptr, dev_targets_ptr, n):
        """Device arrays (drives: uint32, strictly ascending, or None for drives 0..n-1; targets: float64); enqueues only.  An
        entry the host variant would refuse is skipped."""
        _check(hip_lib().xpbd_world_set_drive_targets_device(self._h, C.c_void_p(dev_drives_ptr or None), C.c_void_p(dev_targets_ptr or None), n))

    # kinematic bodies (include/xpbd.h, "KINEMATIC bodies")
    def set_kinematics(self, table):
        """Replaces the kinematic table: KINEMATIC_DTYPE records (see kinematics()), bodies strictly ascending and fixed; None or
        an empty table clears it.  May wait."""
        t = np.zeros(0, dtype=KINEMATIC_DTYPE) if table is None else np.ascontiguousarray(table, dtype=KINEMATIC_DTYPE)
        _check(hip_lib().xpbd_world_set_kinematics(self._h, t.ctypes.data if t.size else None, t.size))

    def set_kinematic_targets(self, entries, rows):
        """Replaces linear and angular (rows of seven doubles) of the listed entries of the last set_kinematics (strictly
        ascending indices; None: all of them) and leaves body and mode.  Waits; wakes nobody."""
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 7)
        idx = None if entries is None else np.ascontiguousarray(entries, dtype=np.uint32)
        if idx is not None and idx.size != r.shape[0]:
            raise ValueError("set_kinematic_targets: %d entries but %d rows" % (idx.size, r.shape[0]))
        if idx is not None and idx.size == 0:
            return
        _check(hip_lib().xpbd_world_set_kinematic_targets(self._h, None if idx is None else idx.ctypes.data, r.ctypes.data if r.size else None, r.shape[0]))

    def set_kinematic_targets_device(self, dev_entries_ptr, dev_rows_ptr, n):
        """Device arrays (entries: uint32, strictly ascending, or None for entries 0..n-1; rows: n x 7 float64); enqueues only.
        An entry the host variant would refuse is skipped."""
        _check(hip_lib().xpbd_world_set_kinematic_targets_device(self._h, C.c_void_p(dev_entries_ptr or None), C.c_void_p(dev_rows_ptr or None), n))

    def frame_neighbours(self):
        """(offsets[n+1], neighbours) CSR of the neighbour lists the last step's broadphase built: the frame's pair list, seen
        from both ends.  Downloads only (neighbours() runs a broadphase of its own)."""
        off = np.zeros(self.n + 1, dtype=np.uint32)
        cap = max(64, 16 * self.n)
        while True:
            nb = np.zeros(cap, dtype=np.uint32)
            rc = hip_lib().xpbd_world_download_neighbours(self._h, _u32(off), _u32(nb), cap)
            if rc != E_CAPACITY:
                _check(rc)
                return off, nb[:off[-1]]
            cap *= 4

    def kinematic_count(self):
        return int(hip_lib().xpbd_world_kinematic_count(self._h))

    # sensor bodies (include/xpbd.h, "SENSOR bodies")
    def set_sensors(self, is_sensor):
        """Replaces the sensor table: one byte (0 / 1) per body; None or an empty array clears it.  May wait."""
        t = np.zeros(0, dtype=np.uint8) if is_sensor is None else np.ascontiguousarray(is_sensor, dtype=np.uint8).reshape(-1)
        _check(hip_lib().xpbd_world_set_sensors(self._h, t.ctypes.data if t.size else None, t.size))

    def get_sensors(self):
        out = np.zeros(self.n, dtype=np.uint8)
        _check(hip_lib().xpbd_world_get_sensors(self._h, out.ctypes.data if out.size else None, out.size))
        return out

    def sensor_count(self):
        return int(hip_lib().xpbd_world_sensor_count(self._h))

    def sensor_overlaps(self, cap=None):
        """(sensors, offsets, hits) of the current report frame: hits[offsets[k]:offsets[k + 1]] (SENSOR_HIT_DTYPE) are the bodies
        that touched sensors[k] in the frame, ascending, each with the index of its record in pair_contacts().  cap=None sizes
        the hits to fit; with a cap below the total the call raises XpbdError(E_CAPACITY) -- sensor_overlaps_raw shows the prefix."""
        if cap is None:
            cap = self.sensor_overlaps_raw(0)[4]
        rc, sensors, offsets, hits, total = self.sensor_overlaps_raw(cap)
        _check(rc)
        return sensors, offsets, hits[:total]

    def sensor_overlaps_raw(self, cap):
        """(rc, sensors, offsets, hits[cap], total): the call as it is; rc other than OK or E_CAPACITY raises."""
        k = self.sensor_count()
        sensors, offsets = np.zeros(k, dtype=np.uint32), np.zeros(k + 1, dtype=np.uint32)
        hits = np.zeros(cap, dtype=SENSOR_HIT_DTYPE)
        total = C.c_uint32(0)
        rc = hip_lib().xpbd_world_sensor_overlaps(self._h, sensors.ctypes.data, offsets.ctypes.data, hits.ctypes.data if cap else None, cap,
                                                  C.byref(total))
        if rc != E_CAPACITY:
            _check(rc)
        return rc, sensors, offsets, hits, int(total.value)

    def sensor_overlaps_device(self, dev_sensors_ptr, dev_offsets_ptr, dev_hits_ptr, cap):
        """Device arrays (sensors: sensor_count() uint32, offsets: one more, hits: cap SENSOR_HIT_DTYPE records); enqueues only."""
        _check(hip_lib().xpbd_world_sensor_overlaps_device(self._h, C.c_void_p(dev_sensors_ptr or None), C.c_void_p(dev_offsets_ptr or None),
                                                           C.c_void_p(dev_hits_ptr or None), cap))


def _report_counts(counts_fn, h):
    out = (C.c_uint32 * 4)()
    _check(counts_fn(h, out))
    return tuple(int(v) for v in out)


def _pair_contacts(counts_fn, download_fn, h, points):
    n_pairs, n_points, _, _ = _report_counts(counts_fn, h)
    pairs = np.zeros(n_pairs, dtype=PAIR_CONTACT_DTYPE)
    pts = np.zeros(n_points, dtype=CONTACT_POINT_DTYPE) if points else None
    got_pairs, got_points = C.c_uint32(0), C.c_uint32(0)
    _check(download_fn(h, pairs.ctypes.data if n_pairs else None, n_pairs, pts.ctypes.data if points and n_points else None,
                       n_points if points else 0, C.byref(got_pairs), C.byref(got_points)))
    return pairs, pts


def _contact_events(counts_fn, download_fn, h):
    _, _, begins, ends = _report_counts(counts_fn, h)
    out = np.zeros(begins + ends, dtype=CONTACT_EVENT_DTYPE)
    n = C.c_uint32(0)
    _check(download_fn(h, out.ctypes.data if out.size else None, out.size, C.byref(n)))
    return out


def impulses(body, impulse, point=None, angular_impulse=None):
    """IMPULSE_DTYPE records from bodies, (n, 3) impulses (broadcast), world points (None: at the centre of mass) and angular
    impulses (None: zero)."""
    b = np.atleast_1d(np.asarray(body, dtype=np.uint32))
    out = np.zeros(b.size, dtype=IMPULSE_DTYPE)
    out["body"], out["impulse"] = b, impulse
    if point is None:
        out["flags"] = IMPULSE_AT_CENTRE
    else:
        out["point"] = point
    if angular_impulse is not None:
        out["angular_impulse"] = angular_impulse
    return out


def _set_wrench(fn, h, indices, force, torque):
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    f = None if force is None else np.ascontiguousarray(force, dtype=np.float64).reshape(-1, 3)
    t = None if torque is None else np.ascontiguousarray(torque, dtype=np.float64).reshape(-1, 3)
    n = idx.size if idx is not None else (f if f is not None else t).shape[0] if (f is not None or t is not None) else 0
    for a in (f, t):
        if a is not None and a.shape[0] != n:
            raise ValueError("force / torque need one row per listed body")
    return fn(h, None if idx is None else idx.ctypes.data, n, None if f is None else f.ctypes.data, None if t is None else t.ctypes.data)


def _filters(filters):
    """COLLISION_FILTER_DTYPE records from records or an (n, 2) array of (group, mask); None stays None."""
    if filters is None:
        return None
    f = np.asarray(filters)
    if f.dtype != COLLISION_FILTER_DTYPE:
        f = np.ascontiguousarray(f, dtype=np.uint32).reshape(-1, 2).view(COLLISION_FILTER_DTYPE).reshape(-1)
    return np.ascontiguousarray(f)


def _materials(materials):
    """MATERIAL_DTYPE records from records or an array of friction coefficients; None stays None."""
    if materials is None:
        return None
    m = np.asarray(materials)
    if m.dtype != MATERIAL_DTYPE:
        rec = np.zeros(m.size, dtype=MATERIAL_DTYPE)
        rec["friction"] = np.asarray(m, dtype=np.float64).reshape(-1)
        m = rec
    return np.ascontiguousarray(m)


def polytope_descs(polytopes):
    """(xpbd_polytope array, the numpy arrays it points into) from a list of polytope dicts."""
    keep, descs = [], (PolytopeDesc * len(polytopes))()
    for d, p in zip(descs, polytopes):
        v = np.ascontiguousarray(p["vertices"], dtype=np.float64).reshape(-1, 3)
        e = np.ascontiguousarray(p["edges"], dtype=np.uint32).reshape(-1, 2)
        fo = np.ascontiguousarray(p["face_offsets"], dtype=np.uint32)
        fi = np.ascontiguousarray(p["face_indices"], dtype=np.uint32)
        keep += [v, e, fo, fi]
        d.vertices_xyz, d.edges, d.face_offsets, d.face_indices = _f64(v), _u32(e), _u32(fo), _u32(fi)
        d.n_vertices, d.n_edges, d.n_faces = v.shape[0], e.shape[0], fo.size - 1
        d.centroid[:] = [float(x) for x in p["centroid"]]
    return descs, keep


def pile_depth(count, pitch, layers):
    """Extent in y (metres, one pitch of clearance included) of a scene_pile of `count` bodies: piles laid side by side at
    this spacing form one continuous pile."""
    per_layer = (count + layers - 1) // layers
    w = default_grid_width(per_layer)
    return pitch * ((per_layer + w - 1) // w)


def comm_library():
    """Path of the RCCL library the multi-GPU world is bound to (None if none could be loaded)."""
    L = hip_lib()
    L.xpbd_comm_library.restype = C.c_char_p
    p = L.xpbd_comm_library()
    return p.decode() if p else None


def comm_unique_id():
    """XPBD_COMM_ID_BYTES of a fresh RCCL communicator id (made on one rank, handed to all)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(hip_lib().xpbd_comm_unique_id(buf))
    return buf.raw


class MultiWorld:
    """xpbd_multi_world: this process's local shards of an N-body world with body-body contacts sharded over n_ranks GPUs
    (EXTENSION; the caller is World::integrate, src/world.rs:34-43)."""

    def __init__(self, n_ranks, first_rank=0, devices=(0,), transport=TRANSPORT_RCCL, comm_id=None, pad=0.02, halo_margin=0.5,
                 narrowphase=NARROWPHASE_SAT, auto_replan=False, plan_through_device=False, full_plans=False):
        L = hip_lib()
        cfg = MultiConfig()
        L.xpbd_multi_config_default(C.byref(cfg))
        self._devices = (C.c_int32 * len(devices))(*devices)
        self._comm_id = comm_id
        cfg.n_ranks, cfg.first_rank, cfg.n_local, cfg.devices = n_ranks, first_rank, len(devices), self._devices
        cfg.transport, cfg.comm_id = transport, comm_id
        cfg.flags = (MULTI_AUTO_REPLAN if auto_replan else 0) | (MULTI_PLAN_THROUGH_DEVICE if plan_through_device else 0) \
            | (MULTI_FULL_PLANS if full_plans else 0)
        cfg.contact_pad, cfg.halo_margin, cfg.narrowphase = pad, halo_margin, narrowphase
        self._h = C.c_void_p()
        _check(L.xpbd_multi_world_create(C.byref(self._h), C.byref(cfg)))
        self.n = self.n_global = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            hip_lib().xpbd_multi_world_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_polytopes(self, polytopes):
        descs, _keep = polytope_descs(polytopes)
        _check(hip_lib().xpbd_multi_world_set_polytopes(self._h, descs, len(polytopes)))

    def set_max_depenetration_speed(self, speed):
        _check(hip_lib().xpbd_multi_world_set_max_depenetration_speed(self._h, speed))

    def set_joint_limits(self, limits):
        """limits: JOINT_LIMIT_DTYPE records naming joints of the last upload by their global index (empty clears them)."""
        lim = np.ascontiguousarray(limits, dtype=JOINT_LIMIT_DTYPE)
        _check(hip_lib().xpbd_multi_world_set_joint_limits(self._h, lim.ctypes.data if lim.size else None, lim.size))

    def set_joint_drives(self, drives):
        """drives: JOINT_DRIVE_DTYPE records naming joints of the last upload by their global index (empty clears them)."""
        drv = np.ascontiguousarray(drives, dtype=JOINT_DRIVE_DTYPE)
        _check(hip_lib().xpbd_multi_world_set_joint_drives(self._h, drv.ctypes.data if drv.size else None, drv.size))

    def set_collision_filters(self, filters=None, flags=0):
        """World.set_collision_filters over the whole sharded world: n_global records in global body order (not collective)."""
        f = _filters(filters)
        _check(hip_lib().xpbd_multi_world_set_collision_filters(self._h, None if f is None else f.ctypes.data, 0 if f is None else f.size,
                                                                flags))

    def set_materials(self, materials=None, ground_friction=np.inf):
        """World.set_materials over the whole sharded world: n_global records in global body order (not collective)."""
        m = _materials(materials)
        _check(hip_lib().xpbd_multi_world_set_materials(self._h, None if m is None else m.ctypes.data, 0 if m is None else m.size,
                                                        ground_friction))

    def set_external_wrench(self, indices=None, force=None, torque=None):
        """World.set_external_wrench with GLOBAL body indices (not collective: every rank passes the same list)."""
        _check(_set_wrench(hip_lib().xpbd_multi_world_set_external_wrench, self._h, indices, force, torque))

    def apply_impulses(self, impulses):
        """World.apply_impulses with GLOBAL bodies (not collective: every rank passes the same list)."""
        imp = np.ascontiguousarray(impulses, dtype=IMPULSE_DTYPE).reshape(-1)
        _check(hip_lib().xpbd_multi_world_apply_impulses(self._h, imp.ctypes.data if imp.size else None, imp.size))

    def upload(self, bodies, shape_id, first_global, n_global, joints=None):
        """bodies / shape_id: the slice of the caller's bodies this process hands over, global indices [first_global,
        first_global + len), in any order: the library decides who owns what."""
        b = np.ascontiguousarray(bodies, dtype=np.float64).reshape(-1, RIGID_DOUBLES)
        sid = None if shape_id is None else np.ascontiguousarray(shape_id, dtype=np.uint32)
        j = np.zeros(0, dtype=JOINT_DTYPE) if joints is None else np.ascontiguousarray(joints, dtype=JOINT_DTYPE)
        _check(hip_lib().xpbd_multi_world_upload(self._h, b.ctypes.data, None if sid is None else _u32(sid), first_global, b.shape[0],
                                                 n_global, j.ctypes.data if j.size else None, j.size))
        self.n, self.n_global = b.shape[0], n_global

    def step(self, dt, substeps):
        _check(hip_lib().xpbd_multi_world_step(self._h, dt, substeps))

    def replan(self):
        _check(hip_lib().xpbd_multi_world_replan(self._h))

    def raycast(self, rays, flags=0, mask=None):
        """World.raycast over the whole sharded world (collective); bodies and ignore_body are global indices."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        out = np.zeros(r.size, dtype=RAY_HIT_DTYPE)
        rp, hp = r.ctypes.data if r.size else None, out.ctypes.data if r.size else None
        if mask is None:
            _check(hip_lib().xpbd_multi_world_raycast(self._h, rp, r.size, flags, hp))
        else:
            _check(hip_lib().xpbd_multi_world_raycast_masked(self._h, rp, r.size, flags, mask, hp))
        return out

    def overlap(self, queries, flags=0):
        """World.overlap over the whole sharded world (collective); bodies and ignore_body are global indices."""
        return _overlap(hip_lib().xpbd_multi_world_overlap, self._h, queries, flags)

    def sweep(self, sweeps, flags=0):
        """World.sweep over the whole sharded world (collective); bodies and ignore_body are global indices."""
        return _sweep(hip_lib().xpbd_multi_world_sweep, self._h, sweeps, flags)

    def distance(self, queries, flags=0):
        """World.distance over the whole sharded world (collective); bodies and ignore_body are global indices."""
        return _distance(hip_lib().xpbd_multi_world_distance, self._h, queries, flags)

    def synchronize(self):
        _check(hip_lib().xpbd_multi_world_synchronize(self._h))

    def download(self):
        out = np.empty((self.n, RIGID_DOUBLES), dtype=np.float64)
        _check(hip_lib().xpbd_multi_world_download(self._h, out.ctypes.data, self.n))
        return out

    def download_owned(self):
        """(global ids, (k, 38) states) of the bodies this process's shards own at the moment.  Not collective."""
        n = C.c_uint32(0)
        cap = max(self.n_global, 1)
        ids, out = np.empty(cap, dtype=np.uint32), np.empty((cap, RIGID_DOUBLES), dtype=np.float64)
        _check(hip_lib().xpbd_multi_world_download_owned(self._h, _u32(ids), out.ctypes.data, cap, C.byref(n)))
        return ids[: n.value].copy(), out[: n.value].copy()

    def plan_stats(self):
        """dict: plans, frames undone, bodies that changed owner at the last plan, fewest / most bodies owned by a rank, step
        calls and the host nanoseconds inside them (enqueueing, waiting for the pair counts, waiting for the frame's end), and the
        host nanoseconds spent in plans (creation, re-plans)."""
        out = (C.c_uint64 * 12)()
        _check(hip_lib().xpbd_multi_world_plan_stats(self._h, out))
        keys = ("plans", "rollbacks", "migrated", "owned_min", "owned_max", "steps", "ns_enqueue", "ns_wait_broadphase", "ns_wait_frame", "ns_plan",
                "full_plans", "light_plans")
        return dict(zip(keys, (int(x) for x in out)))

    def owners(self):
        out = np.empty(self.n_global, dtype=np.uint8)
        _check(hip_lib().xpbd_multi_world_owners(self._h, out.ctypes.data, self.n_global))
        return out

    def halo_stats(self):
        """dict: bodies of the world, owned / ghost / boundary bodies here, rows per rank of the all-gather, plans made, and
        the largest distance a body had travelled at the last check."""
        out, moved = (C.c_uint64 * 6)(), C.c_double(0.0)
        _check(hip_lib().xpbd_multi_world_halo_stats(self._h, out, C.byref(moved)))
        keys = ("bodies_global", "owned", "ghosts", "boundary", "rows_per_rank", "plans")
        return dict(zip(keys, (int(x) for x in out)), max_displacement=moved.value)

    def contact_stats(self):
        out = (C.c_uint64 * 3)()
        _check(hip_lib().xpbd_multi_world_contact_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    # contact reports of the whole sharded world, global body indices (include/xpbd.h, "Contact REPORTS"); gathered by step()
    def set_contact_report(self, enable):
        _check(hip_lib().xpbd_multi_world_set_contact_report(self._h, 1 if enable else 0))

    def contact_report_counts(self):
        return _report_counts(hip_lib().xpbd_multi_world_contact_report_counts, self._h)

    def pair_contacts(self, points=True):
        L = hip_lib()
        return _pair_contacts(L.xpbd_multi_world_contact_report_counts, L.xpbd_multi_world_download_pair_contacts, self._h, points)

    def contact_events(self):
        L = hip_lib()
        return _contact_events(L.xpbd_multi_world_contact_report_counts, L.xpbd_multi_world_download_contact_events, self._h)


def halo_cell_key(centre, edge):
    c = np.ascontiguousarray(centre, dtype=np.float64)
    return int(hip_lib().xpbd_halo_cell_key(_f64(c), edge))


def halo_plan(cell_keys, n_ranks, rank, joints=None):
    """(ghost ids, boundary ids) of one rank from the grid-cell keys of ALL bodies: host-only, as xpbd_multi_world_upload plans."""
    keys = np.ascontiguousarray(cell_keys, dtype=np.int64)
    j = np.zeros(0, dtype=JOINT_DTYPE) if joints is None else np.ascontiguousarray(joints, dtype=JOINT_DTYPE)
    ghosts, boundary = np.zeros(len(keys), dtype=np.uint32), np.zeros(len(keys), dtype=np.uint32)
    ng, nb = C.c_uint32(0), C.c_uint32(0)
    _check(hip_lib().xpbd_halo_plan(keys.ctypes.data_as(C.POINTER(C.c_int64)), len(keys), n_ranks, rank, j.ctypes.data if j.size else None,
                                    j.size, _u32(ghosts), C.byref(ng), _u32(boundary), C.byref(nb), len(keys)))
    return ghosts[: ng.value].copy(), boundary[: nb.value].copy()


def halo_partition(cell_keys, n_ranks):
    """owner[g] of every body from the grid-cell keys of ALL bodies: host-only, as xpbd_multi_world_upload cuts the shards."""
    keys = np.ascontiguousarray(cell_keys, dtype=np.int64)
    owner = np.zeros(len(keys), dtype=np.uint8)
    L = hip_lib()
    L.xpbd_halo_partition.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    _check(L.xpbd_halo_partition(keys.ctypes.data, len(keys), n_ranks, owner.ctypes.data))
    return owner


def halo_plan_owned(cell_keys, owner, n_ranks, rank, joints=None, with_far=False):
    """(ghost ids, boundary ids[, far flags per owned body]) of one rank from the cell keys and owners of ALL bodies."""
    keys = np.ascontiguousarray(cell_keys, dtype=np.int64)
    own = np.ascontiguousarray(owner, dtype=np.uint8)
    j = np.zeros(0, dtype=JOINT_DTYPE) if joints is None else np.ascontiguousarray(joints, dtype=JOINT_DTYPE)
    ghosts, boundary = np.zeros(len(keys), dtype=np.uint32), np.zeros(len(keys), dtype=np.uint32)
    far = np.zeros(len(keys), dtype=np.uint8)
    ng, nb = C.c_uint32(0), C.c_uint32(0)
    L = hip_lib()
    L.xpbd_halo_plan_owned.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, _u32p, _u32p, _u32p,
                                       _u32p, C.c_void_p, C.c_uint32]
    _check(L.xpbd_halo_plan_owned(keys.ctypes.data, own.ctypes.data, len(keys), n_ranks, rank, j.ctypes.data if j.size else None, j.size,
                                  _u32(ghosts), C.byref(ng), _u32(boundary), C.byref(nb), far.ctypes.data if with_far else None, len(keys)))
    if with_far:
        return ghosts[: ng.value].copy(), boundary[: nb.value].copy(), far[: int((own == rank).sum())].copy()
    return ghosts[: ng.value].copy(), boundary[: nb.value].copy()


def halo_plan_light(keys_at_cut, cell_keys, n_ranks, rank, joints=None):
    """(owner of every body now, own ids, ghost ids, boundary ids, far flags) of one rank's LIGHT plan (host only): cuts from
    `keys_at_cut`, owners from `cell_keys` and those cuts, halos from the rank's own bodies and everybody's rims."""
    k0 = np.ascontiguousarray(keys_at_cut, dtype=np.int64)
    k1 = np.ascontiguousarray(cell_keys, dtype=np.int64)
    n = len(k1)
    j = np.zeros(0, dtype=JOINT_DTYPE) if joints is None else np.ascontiguousarray(joints, dtype=JOINT_DTYPE)
    owner = np.zeros(n, dtype=np.uint8)
    own, ghosts, boundary = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    far = np.zeros(n, dtype=np.uint8)
    no, ng, nb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    L = hip_lib()
    L.xpbd_halo_plan_light.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, _u32p, _u32p,
                                       _u32p, _u32p, _u32p, _u32p, C.c_void_p, C.c_uint32]
    _check(L.xpbd_halo_plan_light(k0.ctypes.data, k1.ctypes.data, n, n_ranks, rank, j.ctypes.data if j.size else None, j.size, owner.ctypes.data,
                                  _u32(own), C.byref(no), _u32(ghosts), C.byref(ng), _u32(boundary), C.byref(nb), far.ctypes.data, n))
    return owner, own[: no.value].copy(), ghosts[: ng.value].copy(), boundary[: nb.value].copy(), far[: no.value].copy()


def halo_plan_far(cell_keys, n_ranks, rank):
    """Per owned body of `rank` (index order): 1 if the plan classes it as far from every foreign body (host-only)."""
    keys = np.ascontiguousarray(cell_keys, dtype=np.int64)
    far = np.zeros(len(keys), dtype=np.uint8)
    n = C.c_uint32(0)
    L = hip_lib()
    L.xpbd_halo_plan_far.argtypes = [C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, _u32p]
    _check(L.xpbd_halo_plan_far(keys.ctypes.data_as(C.POINTER(C.c_int64)), len(keys), n_ranks, rank, far.ctypes.data, len(keys), C.byref(n)))
    return far[: n.value].copy()


def step_one(rigid, verts_xyz, dt, substeps):
    """solver::step for one body (src/solver.rs:3) through xpbd_step_one; returns the new 38-double state."""
    r = np.array(rigid, dtype=np.float64).reshape(RIGID_DOUBLES).copy()
    v = np.ascontiguousarray(verts_xyz, dtype=np.float64).reshape(-1)
    _check(hip_lib().xpbd_step_one(r.ctypes.data, _f64(v), v.size // 3, dt, substeps))
    return r


def selftest_div_sqrt(a, b, device=0):
    """(a / b, sqrt(a)) computed on the GPU with the kernels' own compile flags."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    q, s = np.empty_like(a), np.empty_like(a)
    _check(hip_lib().xpbd_selftest_div_sqrt(device, _f64(a), _f64(b), _f64(q), _f64(s), a.size))
    return q, s


def selftest_exact_math(x, a, h, device=0):
    """(fast, plain), each [3, n]: div_by(x, h), then s and k of sqrt_and_reciprocal(a) -- and x / h, sqrt(a), 1 / sqrt(a),
    all computed on the GPU."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if x.shape != a.shape or x.ndim != 1:
        raise ValueError("x and a must be one-dimensional and of one length")
    fast, plain = np.empty((3, x.size)), np.empty((3, x.size))
    _check(hip_lib().xpbd_selftest_exact_math(device, _f64(x), _f64(a), float(h), x.size, _f64(fast), _f64(plain)))
    return fast, plain


def selftest_gather(records, record_bytes, read_bytes, repeats=5, device=0):
    """GB/s of a gather of known size (every record read once, 16-byte loads): the FETCH_SIZE calibration kernel."""
    out = C.c_double(0.0)
    L = hip_lib()
    L.xpbd_selftest_gather.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _f64p]
    _check(L.xpbd_selftest_gather(device, records, record_bytes, read_bytes, repeats, C.byref(out)))
    return out.value


def selftest_hbm_copy(nbytes=1 << 31, repeats=10, device=0):
    """GB/s (read + written) of a device-to-device copy by the library's streaming kernel: the measured HBM roof."""
    out = C.c_double(0.0)
    _check(hip_lib().xpbd_selftest_hbm_copy(device, nbytes, repeats, C.byref(out)))
    return out.value


def selftest_field_streams(bodies=2097152, tile_major=False, repeats=10, device=0):
    """GB/s of the access pattern of one substep of the pinned path alone (38 doubles in, 13 out per body): the roof of
    XPBD_MODE_PER_SUBSTEP in the world's field-major layout, or in a tile-major one."""
    out = C.c_double(0.0)
    _check(hip_lib().xpbd_selftest_field_streams(device, bodies, 1 if tile_major else 0, repeats, C.byref(out)))
    return out.value


# ---- host mirror (CPU set-up math; no GPU needed) -------------------------------
SAT_SCHEDULE_AUTO, SAT_SCHEDULE_ONE_PASS, SAT_SCHEDULE_TWO_PASS = 0, 1, 2
SCENE_BOXES, SCENE_MIXED, SCENE_BOXES_DROP, SCENE_MIXED_DROP, SCENE_BOX_STACKS = 0, 1, 2, 3, 4
SHAPE_CUBE, SHAPE_TETRAHEDRON, SHAPE_ICOSAHEDRON = 0, 1, 2


def scene_shapes(kind):
    verts = np.zeros(3 * 64)
    off = np.zeros(9, dtype=np.uint32)
    ns = host_lib().xpbdh_scene_shapes(kind, _f64(verts), 64, _u32(off), 8)
    if ns < 0:
        raise XpbdError(E_CAPACITY, "scene shape tables too large")
    off = off[: ns + 1].copy()
    return verts[: 3 * off[-1]].reshape(-1, 3).copy(), off


def default_grid_width(n):
    return int(host_lib().xpbdh_default_grid_width(n))


def scene_generate(kind, seed, n, first=0, count=None, grid_w=None):
    """Bodies [first, first+count) of the n-body seeded scene: ((count,38) f64, (count,) u32)."""
    count = n - first if count is None else count
    grid_w = default_grid_width(n) if grid_w is None else grid_w
    bodies = np.zeros((count, RIGID_DOUBLES))
    sid = np.zeros(count, dtype=np.uint32)
    rc = host_lib().xpbdh_scene_generate(kind, seed, grid_w, first, count, bodies.ctypes.data, _u32(sid))
    if rc != OK:
        raise XpbdError(rc, "scene generation failed")
    return bodies, sid


def scene_pile(kind, seed, n, pitch, layers, layer_gap=2.5, lift=0.6, first=0, count=None, y_offset=0.0):
    """The seeded scene re-gridded into a PILE for the body-body contact extension: `layers` layers of a square grid at
    `pitch` metres, `layer_gap` metres apart, the CENTRES OF MASS on the grid points (world centre = position +
    center_of_mass whatever the rotation, src/rigid.rs:75-80; the shapes' origins are a corner for the cube and the
    tetrahedron and the centre for the icosahedron), heights lifted by `lift`.  With the defaults nothing overlaps at
    t = 0: cube radius 0.866 about its centre, half-size tetrahedron 0.42, icosahedron 0.5; the generator's heights jitter by
    0.6 m; the mixed grid never puts two cubes side by side when the grid width is not a multiple of 3 (shape = index
    mod 3) and pitch >= 1.4 keeps a cube clear of the smaller shapes; boxes need pitch >= 1.75.  A scene with deep
    initial overlaps is resolved in ONE substep (XPBD has no velocity clamp), i.e. depth / h = 120 m/s for 0.1 m, and
    never reaches a steady contact regime."""
    count = n - first if count is None else count     # bodies [first, first + count) of the n-body seeded scene form the pile
    bodies, sid = scene_generate(kind, seed, n, first=first, count=count)
    per_layer = (count + layers - 1) // layers
    w = default_grid_width(per_layer)
    i = np.arange(count)
    k = i % per_layer
    bodies[:, 31] = pitch * (k % w) - bodies[:, 28]
    bodies[:, 32] = y_offset + pitch * (k // w) - bodies[:, 29]
    bodies[:, 33] += lift + layer_gap * (i // per_layer) + (0.5 - bodies[:, 30])
    return bodies, sid


def rigid_metrics(shape, scale, density):
    out = np.zeros(14)
    host_lib().xpbdh_rigid_metrics(shape, scale, density, _f64(out))
    return out


def rigid_new(metrics):
    out = np.zeros(RIGID_DOUBLES)
    m = np.ascontiguousarray(metrics, dtype=np.float64)
    rc = host_lib().xpbdh_rigid_new(_f64(m), out.ctypes.data)
    if rc != OK:
        raise XpbdError(rc, "Inertia tensor is not invertible")
    return out


def rigid_frame(rigid):
    r = np.ascontiguousarray(rigid, dtype=np.float64)
    out = np.zeros(7)
    host_lib().xpbdh_rigid_frame(r.ctypes.data, _f64(out))
    return out


def world_new():
    a, b = np.zeros(RIGID_DOUBLES), np.zeros(RIGID_DOUBLES)
    rc = host_lib().xpbdh_world_new(a.ctypes.data, b.ctypes.data)
    if rc != OK:
        raise XpbdError(rc, "World::new failed")
    return a, b


def polytope(shape, scale=1.0):
    """Topology of a standard shape (host mirror's Polytope) as the dict World.set_polytopes takes."""
    counts = np.zeros(4, dtype=np.uint32)
    host_lib().xpbdh_polytope_arrays(shape, scale, _u32(counts), None, None, None, None, None)
    v = np.zeros((counts[0], 3))
    e = np.zeros((counts[1], 2), dtype=np.uint32)
    fo = np.zeros(counts[2] + 1, dtype=np.uint32)
    fi = np.zeros(counts[3], dtype=np.uint32)
    c = np.zeros(3)
    host_lib().xpbdh_polytope_arrays(shape, scale, _u32(counts), _f64(v), _u32(e), _u32(fo), _u32(fi), _f64(c))
    return {"vertices": v, "edges": e, "face_offsets": fo, "face_indices": fi, "centroid": c}


def scene_polytopes(kind):
    """Polytopes of a scene kind, in shape-id order (matches scene_shapes)."""
    if not (kind & 1):
        return [polytope(SHAPE_CUBE)]
    return [polytope(SHAPE_CUBE), polytope(SHAPE_TETRAHEDRON, 0.5), polytope(SHAPE_ICOSAHEDRON, 0.5)]


def shape_planes(shape, scale=1.0):
    out = np.zeros(4)
    n = host_lib().xpbdh_shape_plane(shape, scale, 0xFFFFFFFF, _f64(out))
    planes = np.zeros((n, 4))
    for i in range(n):
        host_lib().xpbdh_shape_plane(shape, scale, i, _f64(planes[i]))
    return planes
