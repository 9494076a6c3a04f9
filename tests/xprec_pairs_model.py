"""Extended-precision model of the body-body contact extension: the manifold of a pair (stage N) and one contacts
substep of n bodies (stage S).

A second reading of oracle/xpbd_pairs_oracle.h's prose (steps 1-5, the manifold conventions) and of the reference lines
that header cites; it does not follow xpbd_pairs_oracle.c, the kernels or tests/material_model.py.  Stage N is plain
geometry: every query is a maximum over ALL faces or edge pairs of a minimum over ALL vertices, evaluated in world space
(a rigid motion keeps distances), where the oracle works in A's space, over unique edge directions and with supports.
Stage S uses tests/xprec_model.py's scalar abstraction, cgmath helpers, integrate, ground and derive.  Its joint and limit
entries (joint_terms) are read from include/xpbd.h (XPBD_JOINT_*, XPBD_LIMIT_*), the joint prose of xpbd_pairs_oracle.h and
constraint.rs:6-37, rigid.rs:113-123; they follow neither tests/joint_limit_model.py, the oracle's C nor the kernel.
Stage 6 (bounce) and the terrain (xprec_model.terrain_lookup, xprec_model.ground) are read from include/xpbd.h's sections
"RESTITUTION" and "TERRAIN" alone; tests/restitution_model.py, tests/terrain_model.py, xpbd_step.hpp, xpbd_contacts.hip and
xpbd_restitution.hip were not read for them.
Stage 0 (kinematic_velocities, the overwrite before integrate) and stage 7 (damp) are read from include/xpbd.h's sections
"KINEMATIC bodies" and "DAMPING" alone; tests/damping_model.py, tests/kinematic_model.py, xpbd_damping.hip, xpbd_kinematic.hip
and xpbd_world_contacts.cpp were not read for them.

Vectors are arrays (3, k) of model scalars as in xprec_model.py.  Reference lines are jim-ec/constraint_solver src/*.rs.
"""
import numpy as np

import xprec_model as xm
from xprec_model import conj, cross, dot, frame_apply, frame_delta, matvec, normalize_q, pure, qmul, qrot

EDGE_BIAS = 1e-6          # OP_EDGE_BIAS
MAX_POINTS = 8            # OP_MAX_POINTS
FACE_A, FACE_B, EDGES = 0, 1, 2
# two edges whose directions enclose less than this sine span no axis (the reference's normalize of their cross product
# is NaN only at exactly 0; next to it the axis is noise, and a face axis describes the same contact)
PARALLEL_SIN = 1e-9
MUTATIONS = ("reference_sign", "arm_without_com", "transposed_inertia", "average_by_pairs", "friction_against_distance",
             "tangential_dropped")
# wrong readings of the joint and limit entries of stage S (joint_terms)
JOINT_MUTATIONS = ("joint_sign_a", "anchor_without_com", "joints_from_integrated", "joints_uncounted", "nonbinding_counted",
                   "binding_twice", "hinge_without_compliance", "twist_unprojected", "limit_same_sign",
                   "joint_depenetration_limited", "joint_transposed_inertia")
# wrong readings of a joint's extra entries (xpbd.h, "SLIDERS and joint DRIVES"): sliders, SLIDE limits, drives.  A list of
# its own beside JOINT_MUTATIONS, whose table (test_xprec_joints_oracle.py) names a scene per member.
DRIVE_MUTATIONS = ("slider_keeps_positional", "perpendicular_sign_a", "extras_uncounted", "nonbinding_slide_counted",
                   "drive_without_base_compliance", "clamp_by_h", "clamped_uncounted", "velocity_from_integrated",
                   "extras_from_integrated", "wrap_dropped", "angular_drive_same_sign", "linear_drive_w_without_angular")
# wrong readings of stage 6 (xpbd.h, "RESTITUTION") and of the terrain as ground ("TERRAIN"); the table of
# test_xprec_bounce_oracle.py names a scene per member
BOUNCE_MUTATIONS = ("e_smaller_side", "vn0_post_derive", "threshold_on_vn", "arms_at_integrated", "points_averaged", "one_sweep",
                    "no_give_back", "entries_summed", "idle_counted", "reference_pushed_same_way", "compliance_in_wsum",
                    "ground_before_pairs", "ground_reads_pre_ground", "impulse_arm_in_rest_space", "triangles_swapped",
                    "target_vertical", "d_unnormalised", "plane_beyond_field", "bounce_normal_vertical",
                    "bounce_lookup_at_integrated")
# wrong readings of stage 7 (xpbd.h, "DAMPING") and of the kinematic overwrite ("KINEMATIC bodies"); the table of
# test_xprec_damping_oracle.py names a scene per member
DAMPING_MUTATIONS = ("drag_explicit", "caps_before_drag", "drag_before_dampers", "stage7_before_stage6", "angular_on_linear_result",
                     "neighbour_stage7_velocities", "count_is_terms", "damper_entries_summed", "k_unclamped", "damper_arm_without_com",
                     "wang_unrotated", "anchors_at_integrated", "fixed_body_damped", "cap_per_component", "second_end_same_sign")
KINEMATIC_MUTATIONS = ("dq_conjugate_first", "dq_not_negated", "full_angle", "r_counted_up", "overwrite_after_integrate",
                       "p_frame_origin", "v0_before_overwrite", "velocity_once_per_frame")
# wrong readings of a substep with sleepers (xpbd.h, "SLEEPING", rules (a)-(c)); the table of test_xprec_sleep_oracle.py names a
# scene per member
SLEEP_MUTATIONS = ("sleeper_share_applied", "sleeper_fixed", "record_from_integrated", "record_after_ground", "record_without_com",
                   "stage6_reads_stored_velocity", "sleeper_point_twice", "sleeper_point_uncounted", "sleeper_drag_applied")
SWEEPS = 4                                                               # XPBD_RESTITUTION_SWEEPS
JOINT_DISTANCE, JOINT_HINGE, JOINT_SLIDER = 0, 1, 2                      # XPBD_JOINT_*
LIMIT_HINGE, LIMIT_SWING, LIMIT_TWIST, LIMIT_SLIDE = 0, 1, 2, 3          # XPBD_LIMIT_*
DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY, DRIVE_POSITION, DRIVE_VELOCITY = 0, 1, 2, 3   # XPBD_DRIVE_*


def shape(poly):
    """An oracle_binding.Polytope as the model's shape: f64 vertices (V, 3), edges (E, 2), a list of face index arrays,
    the centroid."""
    nv, ne, nf = int(poly.n_vertices), int(poly.n_edges), int(poly.n_faces)
    off = [int(poly.face_offsets[i]) for i in range(nf + 1)]
    idx = [int(poly.face_indices[i]) for i in range(off[-1])]
    return {"verts": poly.verts(), "edges": np.array([[poly.edges[i][0], poly.edges[i][1]] for i in range(ne)], dtype=np.int64),
            "faces": [np.array(idx[off[i]:off[i + 1]]) for i in range(nf)], "centroid": poly.centroid.np(),
            "radius": float(np.linalg.norm(poly.verts() - poly.centroid.np(), axis=1).max())}


def _unit(num, v):
    return v / num.sqrt(dot(v, v))


def _world(num, frame, sh):
    """World vertices (3, V), face normals (3, F) and displacements (F,) (Plane::from_points, geometry.rs:16-25, of the
    face's first three vertices, pointing away from the centroid) and the centroid of a shape under a frame (position (3,), rotation (4,))."""
    p, q = frame
    w = frame_apply(p[:, None], q[:, None], num.conv(sh["verts"].T))
    first = np.array([f[:3] for f in sh["faces"]])
    p0, p1, p2 = w[:, first[:, 0]], w[:, first[:, 1]], w[:, first[:, 2]]
    normal = _unit(num, cross(p1 - p0, p2 - p0))
    centroid = frame_apply(p[:, None], q[:, None], num.conv(sh["centroid"][:, None]))
    inward = (dot(normal, centroid - p0) > 0).astype(bool)             # Polytope::plane, geometry.rs:262-271: away from it
    normal = np.where(inward, -normal, normal)
    return w, normal, dot(normal, p0), centroid


def _runner_up(num, values, best):
    rest = np.delete(num.to_f64(values - values[best]), best)
    return float(-rest.max()) if len(rest) else np.inf


def _face_query(num, normal, disp, other):
    """face_axes_separation (collision.rs:123-149): max over the faces of the min over the other body's vertices of the
    plane distance; first maximum.  Returns (value, face, gap to the runner-up face)."""
    dist = (normal[0][:, None] * other[0][None] + normal[1][:, None] * other[1][None] + normal[2][:, None] * other[2][None]
            - disp[:, None])
    depth = dist.min(axis=1)
    best = int(np.argmax(depth))
    return depth[best], best, _runner_up(num, depth, best), depth


def _edge_query(num, wa, wb, ea, eb, centroid_a):
    """edge_axes_separation (collision.rs:151-197) over all E_A x E_B pairs: the normalised cross product, oriented away
    from A's centroid (collision.rs:176-179), separates by min_B - max_A of the projections.  Returns (value or None,
    axis, (edge of A, edge of B), (every pair's value, every pair's axis) in f64)."""
    da, db = wa[:, ea[:, 1]] - wa[:, ea[:, 0]], wb[:, eb[:, 1]] - wb[:, eb[:, 0]]
    foot = wa[:, ea[:, 0]] - centroid_a[:, None]
    best, best_axis, best_pair = None, None, None
    seps, axes = [], []
    for i in range(ea.shape[0]):
        axis = cross(da[:, i:i + 1], db)                                                 # (3, E_B)
        sin2 = dot(axis, axis) / (dot(da[:, i], da[:, i]) * dot(db, db))
        ok = np.nonzero(num.to_f64(sin2) > PARALLEL_SIN ** 2)[0]
        if not len(ok):
            continue
        axis = _unit(num, axis[:, ok])
        flip = (dot(axis, foot[:, i:i + 1]) < 0).astype(bool)
        axis = np.where(flip, -axis, axis)
        proj_a = axis[0][:, None] * wa[0][None] + axis[1][:, None] * wa[1][None] + axis[2][:, None] * wa[2][None]
        proj_b = axis[0][:, None] * wb[0][None] + axis[1][:, None] * wb[1][None] + axis[2][:, None] * wb[2][None]
        sep = proj_b.min(axis=1) - proj_a.max(axis=1)
        seps.append(num.to_f64(sep))
        axes.append(num.to_f64(axis))
        k = int(np.argmax(sep))
        if best is None or sep[k] > best:
            best, best_axis, best_pair = sep[k], axis[:, k], (i, int(ok[k]))
    every = (np.concatenate(seps), np.concatenate(axes, axis=1)) if seps else (np.zeros(0), np.zeros((3, 0)))
    return best, best_axis, best_pair, every


def _supporting_edge(num, w, edges, direction, axis, sign):
    """Among the edges parallel to `direction`, the one furthest along sign * axis (by its midpoint)."""
    d = w[:, edges[:, 1]] - w[:, edges[:, 0]]
    c = cross(d, direction[:, None])
    parallel = num.to_f64(dot(c, c) / (dot(d, d) * dot(direction, direction))) <= PARALLEL_SIN ** 2
    mid = dot(w[:, edges[:, 0]] + w[:, edges[:, 1]], axis[:, None]) * sign
    mid = np.where(parallel, num.to_f64(mid), -np.inf)
    return int(np.argmax(mid))


def _closest_on_segments(num, a0, a1, b0, b1):
    """Closest points of two segments whose lines are not parallel: the lines' closest points, clamped to the segments."""
    u, v, r = a1 - a0, b1 - b0, a0 - b0
    uu, uv, vv, ur, vr = dot(u, u), dot(u, v), dot(v, v), dot(u, r), dot(v, r)
    den = uu * vv - uv * uv
    one, zero = uu * 0 + 1, uu * 0
    s = min(max((uv * vr - vv * ur) / den, zero), one)
    t = min(max((uv * s + vr) / vv, zero), one)
    s = min(max((uv * t - ur) / uu, zero), one)
    return a0 + u * s, b0 + v * t


def _clip(num, poly, ref_poly, ref_normal):
    """Sutherland-Hodgman: the polygon (list of (3,) points) against the side planes of the reference face, the planes
    through its edges along its normal; a point on a plane is inside.  Returns (polygon, smallest non-zero |distance| of a
    tested vertex from a side plane)."""
    margin = np.inf
    centre = sum(ref_poly[1:], ref_poly[0]) / len(ref_poly)
    for k in range(len(ref_poly)):
        if not poly:
            break
        e0, e1 = ref_poly[k], ref_poly[(k + 1) % len(ref_poly)]
        side = _unit(num, cross(e1 - e0, ref_normal))
        if dot(side, centre - e0) > 0:                                  # outward, whichever way the face is wound
            side = -side
        d = [dot(side, p - e0) for p in poly]
        margin = min([margin] + [abs(float(x)) for x in d if x != 0])
        out = []
        for m in range(len(poly)):
            p, q, dp, dq = poly[m], poly[(m + 1) % len(poly)], d[m], d[(m + 1) % len(poly)]
            if dp <= 0:
                out.append(p)
            if (dp < 0 and dq > 0) or (dp > 0 and dq < 0):
                out.append(p + (q - p) * (dp / (dp - dq)))
        poly = out
    return poly, margin


def manifold(frame_a, frame_b, sh_a, sh_b, num=None):
    """Stage N.  frames: (position (3,), rotation (4,)) in model scalars or f64.  Returns a dict: separated, feature,
    index_a, index_b (faces as in op_manifold; for EDGES the undirected vertex pairs edge_a, edge_b instead), separation
    (the chosen feature's query),
    query (a, b, e or None), p_ref and p_inc (lists of (3,) points) and `margins`: touch (|separation|), ab (|a - b|),
    edge (|e - max(a, b) - bias|), ref_face and inc_face (gap to the runner-up: metres, cosine), clip (smallest non-zero
    distance of a clip vertex from a side plane or of a clipped point from the reference plane), axis (how far the best
    query leads the best other axis).  `axis` is the largest query's axis from A towards B, `depth` minus that query."""
    num = num or xm.native()
    fa = (np.asarray(frame_a[0]), np.asarray(frame_a[1]))
    fb = (np.asarray(frame_b[0]), np.asarray(frame_b[1]))
    if fa[0].dtype == np.float64:
        fa, fb = (num.conv(fa[0]), num.conv(fa[1])), (num.conv(fb[0]), num.conv(fb[1]))
    wa, na, da, ca = _world(num, fa, sh_a)
    wb, nb, db, _ = _world(num, fb, sh_b)
    a, face_a, gap_a, all_a = _face_query(num, na, da, wb)
    b, face_b, gap_b, all_b = _face_query(num, nb, db, wa)
    e, axis, pair, (edge_seps, edge_axes) = _edge_query(num, wa, wb, sh_a["edges"], sh_b["edges"], ca[:, 0])
    faces = max(a, b)
    sep = faces if e is None else max(faces, e)
    margins = {"touch": abs(float(sep)), "ab": abs(float(a - b)), "edge": np.inf if e is None else abs(float(e - faces) - EDGE_BIAS),
               "ref_face": np.inf, "inc_face": np.inf, "clip": np.inf}
    # the axis of the largest query, from A towards B, and how far the next other axis is behind it (metres)
    if e is not None and e > faces:
        best_axis = axis
    else:
        best_axis = na[:, face_a] if a >= b else -nb[:, face_b]
    values = np.concatenate([num.to_f64(all_a), num.to_f64(all_b), edge_seps])
    axes = np.concatenate([num.to_f64(na), -num.to_f64(nb), edge_axes], axis=1)
    other = np.abs(num.to_f64(best_axis) @ axes) < 1 - 1e-9
    unique = float(sep) - values[other].max() if other.any() else np.inf
    margins["axis"] = unique
    out = {"separated": bool(sep >= 0), "separation": faces, "axis": best_axis, "depth": -sep, "query": (a, b, e),
           "margins": margins, "p_ref": [], "p_inc": [], "face_axes": (num.to_f64(na), -num.to_f64(nb)),
           "feature": None, "index_a": None, "index_b": None}
    if out["separated"]:
        return out
    if e is not None and e - faces > EDGE_BIAS:                          # the edge pair must beat both faces by the bias
        i = _supporting_edge(num, wa, sh_a["edges"], wa[:, sh_a["edges"][pair[0], 1]] - wa[:, sh_a["edges"][pair[0], 0]], axis, 1)
        j = _supporting_edge(num, wb, sh_b["edges"], wb[:, sh_b["edges"][pair[1], 1]] - wb[:, sh_b["edges"][pair[1], 0]], axis, -1)
        ea, eb = sh_a["edges"][i], sh_b["edges"][j]
        pa, pb = _closest_on_segments(num, wa[:, ea[0]], wa[:, ea[1]], wb[:, eb[0]], wb[:, eb[1]])
        out.update(separation=e, feature=EDGES, edge_a=frozenset(int(x) for x in ea), edge_b=frozenset(int(x) for x in eb), p_ref=[pa], p_inc=[pb])
        return out
    if a >= b:                                                           # the reference face goes to A on a tie
        feature, rf, gap, w_ref, n_ref, d_ref, sh_ref, w_inc, n_inc, sh_inc = FACE_A, face_a, gap_a, wa, na, da, sh_a, wb, nb, sh_b
    else:
        feature, rf, gap, w_ref, n_ref, d_ref, sh_ref, w_inc, n_inc, sh_inc = FACE_B, face_b, gap_b, wb, nb, db, sh_b, wa, na, sh_a
    normal, disp = n_ref[:, rf], d_ref[rf]
    cosines = dot(n_inc, normal[:, None])                                # collision.rs:76-85, first minimum
    inc = int(np.argmin(cosines))
    margins["ref_face"], margins["inc_face"] = gap, _runner_up(num, -cosines, inc)
    poly, clip = _clip(num, [w_inc[:, v] for v in sh_inc["faces"][inc]], [w_ref[:, v] for v in sh_ref["faces"][rf]], normal)
    for p in poly:
        depth = dot(normal, p) - disp
        if depth != 0:
            clip = min(clip, abs(float(depth)))
        if depth < 0:                                                    # strictly below the reference plane
            out["p_inc"].append(p)
            out["p_ref"].append(p - normal * depth)                      # Plane::project, geometry.rs:45-47
    margins["clip"] = clip
    out.update(feature=feature, index_a=rf if feature == FACE_A else inc, index_b=inc if feature == FACE_A else rf,
               normal=normal)                                            # the reference plane's: out of the reference body
    return out


def decided(m, tau):
    """No discrete decision of the manifold has a margin in (0, tau]: an exact tie is decided by the stated rule."""
    g = m["margins"]
    keys = ("touch",) if m["separated"] else (("touch", "edge") if m["feature"] == EDGES else
                                              ("touch", "ab", "edge", "ref_face", "inc_face", "clip"))
    return not any(0 < g[k] <= tau for k in keys)


def manifold_points(manifolds):
    """Flat contact list of stage S from {(i, j): stage N result}: (inc, ref, pair, p_inc (3, P), p_ref (3, P))."""
    inc, ref, pair, p_inc, p_ref = [], [], [], [], []
    for k, ((i, j), m) in enumerate(sorted(manifolds.items())):
        if m["separated"]:
            continue
        r, c = (j, i) if m["feature"] == FACE_B else (i, j)             # reference body: A for FACE_A and EDGES
        for pr, pi in zip(m["p_ref"], m["p_inc"]):
            inc.append(c), ref.append(r), pair.append(k), p_inc.append(pi), p_ref.append(pr)
    return inc, ref, pair, p_inc, p_ref


def joint_terms(num, s, pos, rot, joints, limits, compliance, depenetration=None, mutation=None, drives=(), past=None,
                integrated=None, h=None):
    """The joint entries of stage S's Jacobi pass, all evaluated on the pose (pos, rot) (3, n), (4, n): the pose after
    step 3.  joints / limits: records with the fields of xpbd_joint / xpbd_joint_limit (a limit belongs to `joint`; a joint's
    limits act in the caller's order).  Per joint, each a Jacobi entry of its own on both bodies:
      positional  p = Frame * anchor (frame.rs:47-53, Rigid::frame rigid.rs:75-80: the centre-of-mass offset included);
                  lambda = (|p_b - p_a| - distance) / (w_a + w_b + compliance), w = Constraint::inverse_resitance
                  (constraint.rs:25-32); +lambda dir on a at p_a, -lambda dir on b at p_b as Rigid::apply_impulse
                  (rigid.rs:113-123); no entry when the points coincide exactly.  Never limited by the depenetration speed.
      hinge       (XPBD_JOINT_HINGE) delta = a_w x b_w, n = delta / |delta|, no entry at |delta| = 0; w = the angular half
                  of inverse_resitance; lambda = |delta| / (w + compliance); a turns by +lambda n, b by -lambda n:
                  rotation += 0.5 Quat(0, I^-1 (lambda n)) * rotation.
      limits      SWING, HINGE, TWIST as xpbd.h states them; err = phi - clamp(phi, lower, upper); err == 0 adds nothing,
                  not even to the count; otherwise lambda = err / (w + compliance), turned like the hinge term.
      extras      (xpbd.h, "SLIDERS and joint DRIVES") a SLIDER has the hinge entry and no positional one.  With d = p_b - p_a,
                  a_w = q_a axis_a, s = d . a_w, W(body, p, n) the positional term's w of one body, Wang(n) the limits' w, and
                  a subscript 0 the same expression on `past` = (position, rotation) (3, n), (4, n) at the start of the
                  substep: the perpendicular term r = d - a_w s (|r| = 0: no entry), lambda = |r| / (W_a + W_b + c), +lambda n
                  on a at p_a, -lambda n on b at p_b; the SLIDE limit e = s - clamp(s, lower, upper) (0: nothing), n = a_w,
                  applied alike; then the joint's `drives` (records of xpbd_joint_drive) in the caller's order, e as the
                  header's table, lambda = e / (w + (1e-6 + alpha) / h^2) clamped to +-max_force h^2, w = Wang(a_w) and
                  turned like a limit (angular kinds) or W_a + W_b and pushed like the SLIDE limit (linear kinds).  A joint's
                  extras are summed among themselves and added after its other entries.  `h` in model scalars.
    Returns (sum of position terms (3, n), sum of rotation terms (4, n), count (n,), info): info holds per body n_joint (its
    entries, extras included), n_extra (its extra entries), n_clamped (those whose lambda was clamped), slide_margin
    (smallest |s - bound| of its SLIDE limits, metres), drive_margin (smallest |e| of its drives), drive_wrap_margin
    (smallest |pi - |x|| of the argument x of wrap, which jumps at +-pi), the lists `slides` of (joint, s, e), `perps` of
    (joint, |r|) and `drives` of (index in the caller's list, kind, e, clamped, phi or s), n_binding (its binding limits),
    limit_margin (smallest |phi - nearer bound| of its limits, radians), wrap_margin (smallest pi - |phi|) and joint_cond
    (smallest non-zero s, |bisector|, |delta|, |r| or anchor distance: what a direction is normalised by), and per limit the
    list `limits` of (joint, kind, phi, err) in f64."""
    assert mutation is None or mutation in JOINT_MUTATIONS + DRIVE_MUTATIONS
    sqrt = num.sqrt
    im, M, com = s["inverse_mass"], s["inverse_inertia"], s["center_of_mass"]
    n = pos.shape[1]
    sum_p, sum_q, count = pos * 0, rot * 0, np.zeros(n, dtype=np.int64)
    info = {"n_joint": np.zeros(n, dtype=np.int64), "n_binding": np.zeros(n, dtype=np.int64), "limit_margin": np.full(n, np.inf),
            "wrap_margin": np.full(n, np.inf), "joint_cond": np.full(n, np.inf), "limits": [],
            "n_extra": np.zeros(n, dtype=np.int64), "n_clamped": np.zeros(n, dtype=np.int64), "slide_margin": np.full(n, np.inf),
            "drive_margin": np.full(n, np.inf), "drive_wrap_margin": np.full(n, np.inf), "slides": [], "perps": [], "drives": []}
    by_joint = [[] for _ in range(len(joints))]
    for lim in limits:
        by_joint[int(lim["joint"])].append(lim)
    drives_of = [[] for _ in range(len(joints))]
    for index, drv in enumerate(drives):
        drives_of[int(drv["joint"])].append((index, drv))
    # the poses the extras are read at: those of every other joint entry
    e_pos, e_rot = integrated if mutation == "extras_from_integrated" else (pos, rot)

    def vec(x):
        return num.conv(np.asarray(x, dtype=np.float64))

    def as_float(x):
        return float(num.to_f64(np.array([x]))[0])

    def inertia(body):
        """I^-1 of the body, [column, row].  (The mutation transposes it wherever a joint entry uses it: in w alone, a
        quadratic form, the transpose is the same number.)"""
        return M[:, :, body].T if mutation == "joint_transposed_inertia" else M[:, :, body]

    def entry(body, dp, turn, counts=1):
        """One entry of `body`: a displacement and an angular displacement I^-1-weighted already (rigid.rs:118-122)."""
        if dp is not None:
            sum_p[:, body] = sum_p[:, body] + dp
        sum_q[:, body] = sum_q[:, body] + qmul(pure(turn) * 0.5, rot[:, body])
        count[body] += 0 if mutation == "joints_uncounted" else counts
        info["n_joint"][body] += 1

    def conditioned(bodies, value):
        v = as_float(value)
        if v != 0:
            for body in bodies:
                info["joint_cond"][body] = min(info["joint_cond"][body], v)

    def angular(a, b, n_axis, error, with_compliance=True, counts=1, same_sign=False):
        """An angular entry about the unit axis n: a turns by +lambda n, b by -lambda n."""
        w = 0
        for body in (a, b):
            local = qrot(conj(rot[:, body]), n_axis)                       # q^-1 n
            w = w + dot(matvec(inertia(body), local), local)
        lam = error / (w + compliance if with_compliance else w)
        entry(a, None, matvec(inertia(a), n_axis * lam), counts)
        entry(b, None, matvec(inertia(b), n_axis * (lam if same_sign else -lam)), counts)

    def anchors(P, Q, jt):
        """World anchors (p_a, p_b) and body origins of a joint on the poses (P, Q)."""
        p, origin = [], []
        for body, anchor in ((int(jt["body_a"]), jt["anchor_a"]), (int(jt["body_b"]), jt["anchor_b"])):
            o = P[:, body] + com[:, body]                                   # the body's origin in the world: position + com
            frame_p = o + qrot(Q[:, body], -com[:, body])                   # Rigid::frame, rigid.rs:75-80
            if mutation == "anchor_without_com":
                frame_p = P[:, body]
            p.append(frame_apply(frame_p, Q[:, body], vec(anchor)))
            origin.append(o)
        return p, origin

    def hinge_phi(Q, a, b, axis_a, ref_a, ref_b):
        """The angle of XPBD_LIMIT_HINGE on the rotations Q."""
        n_axis = qrot(Q[:, a], vec(axis_a))
        r_a, r_b = qrot(Q[:, a], vec(ref_a)), qrot(Q[:, b], vec(ref_b))
        return num.atan2(dot(cross(r_a, r_b), n_axis), dot(r_a, r_b))

    for k, jt in enumerate(joints):
        a, b = int(jt["body_a"]), int(jt["body_b"])
        slider = int(jt["kind"]) == JOINT_SLIDER
        p, origin = anchors(pos, rot, jt)
        diff = p[1] - p[0]                                                  # constraint.rs:13-15, contacts = (p_a, p_b)
        dist = sqrt(dot(diff, diff))
        if not slider:
            conditioned((a, b), dist)
        if dist != 0 and (not slider or mutation == "slider_keeps_positional"):
            direction = diff / dist
            w = 0
            for body, point, o in ((a, p[0], origin[0]), (b, p[1], origin[1])):
                local = qrot(conj(rot[:, body]), cross(point - o, direction))
                w = w + im[body] + dot(matvec(inertia(body), local), local)
            error = dist - vec([jt["distance"]])[0]
            if mutation == "joint_depenetration_limited" and depenetration is not None:
                error = min(max(error, -depenetration), depenetration)
            lam = error / (w + compliance)
            for body, point, o, impulse in ((a, p[0], origin[0], direction * (-lam if mutation == "joint_sign_a" else lam)),
                                            (b, p[1], origin[1], direction * -lam)):
                entry(body, impulse * im[body], cross(matvec(inertia(body), point - o), impulse))
        a_w, b_w = qrot(rot[:, a], vec(jt["axis_a"])), qrot(rot[:, b], vec(jt["axis_b"]))
        if int(jt["kind"]) != JOINT_DISTANCE:                               # HINGE and SLIDER
            delta = cross(a_w, b_w)
            mag = sqrt(dot(delta, delta))
            conditioned((a, b), mag)
            if mag != 0:
                angular(a, b, delta / mag, mag, with_compliance=mutation != "hinge_without_compliance")
        for lim in by_joint[k]:
            kind = int(lim["kind"])
            if kind == LIMIT_SLIDE:                                         # the slider rule, among the extras below
                continue
            if kind == LIMIT_SWING:
                c = cross(a_w, b_w)
                sine = sqrt(dot(c, c))
                conditioned((a, b), sine)
                if sine == 0:
                    continue
                phi, n_axis = num.atan2(sine, dot(a_w, b_w)), c / sine
            else:
                r_a, r_b = qrot(rot[:, a], vec(lim["ref_a"])), qrot(rot[:, b], vec(lim["ref_b"]))
                if kind == LIMIT_HINGE:
                    n_axis = a_w
                else:
                    assert kind == LIMIT_TWIST
                    bisector = a_w + b_w
                    length = sqrt(dot(bisector, bisector))
                    conditioned((a, b), length)
                    if length == 0:
                        continue
                    n_axis = bisector / length
                    if mutation != "twist_unprojected":
                        r_a, r_b = r_a - n_axis * dot(r_a, n_axis), r_b - n_axis * dot(r_b, n_axis)
                phi = num.atan2(dot(cross(r_a, r_b), n_axis), dot(r_a, r_b))
            lower, upper = vec([lim["lower"], lim["upper"]])
            error = phi - min(max(phi, lower), upper)
            phi64 = as_float(phi)
            info["limits"].append((k, kind, phi64, as_float(error)))
            for body in (a, b):
                info["limit_margin"][body] = min(info["limit_margin"][body], abs(as_float(phi - lower)),
                                                 abs(as_float(phi - upper)))
                info["wrap_margin"][body] = min(info["wrap_margin"][body], np.pi - abs(phi64))
            if error == 0:
                if mutation == "nonbinding_counted":
                    count[a] += 1
                    count[b] += 1
                continue
            info["n_binding"][[a, b]] += 1
            angular(a, b, n_axis, error, counts=2 if mutation == "binding_twice" else 1, same_sign=mutation == "limit_same_sign")
        # ---- the joint's extra entries, summed among themselves from 0 -------------------------------------------------------
        slides = [lim for lim in by_joint[k] if int(lim["kind"]) == LIMIT_SLIDE]
        if not (slider or slides or drives_of[k]):
            continue
        ex_p = {a: pos[:, a] * 0, b: pos[:, b] * 0}
        ex_q = {a: rot[:, a] * 0, b: rot[:, b] * 0}
        ex_n, ex_entries = {a: 0, b: 0}, {a: 0, b: 0}
        p, origin = anchors(e_pos, e_rot, jt)
        n_axis = qrot(e_rot[:, a], vec(jt["axis_a"]))                       # a_w
        d = p[1] - p[0]
        travel = dot(d, n_axis)                                             # s

        def extra(body, dp, turn, counted=True):
            if dp is not None:
                ex_p[body] = ex_p[body] + dp
            ex_q[body] = ex_q[body] + qmul(pure(turn) * 0.5, e_rot[:, body])
            ex_n[body] += 1 if counted else 0
            ex_entries[body] += 1

        def w_linear(direction, angular_half=True):
            w = 0
            for body, point, o in ((a, p[0], origin[0]), (b, p[1], origin[1])):
                w = w + im[body]
                if angular_half:
                    local = qrot(conj(e_rot[:, body]), cross(point - o, direction))
                    w = w + dot(matvec(inertia(body), local), local)
            return w

        def w_angular(direction):
            w = 0
            for body in (a, b):
                local = qrot(conj(e_rot[:, body]), direction)
                w = w + dot(matvec(inertia(body), local), local)
            return w

        def push(direction, lam, counted=True, sign_a=1):
            """+lambda direction on a at p_a, -lambda direction on b at p_b (Rigid::apply_impulse)."""
            for body, point, o, impulse in ((a, p[0], origin[0], direction * (lam * sign_a)), (b, p[1], origin[1], direction * -lam)):
                extra(body, impulse * im[body], cross(matvec(inertia(body), point - o), impulse), counted)

        if slider:                                                          # 1. the perpendicular term
            r = d - n_axis * travel
            length = sqrt(dot(r, r))
            conditioned((a, b), length)
            info["perps"].append((k, as_float(length)))
            if length != 0:
                direction = r / length
                push(direction, length / (w_linear(direction) + compliance), sign_a=-1 if mutation == "perpendicular_sign_a" else 1)
        for lim in slides:                                                  # 2. XPBD_LIMIT_SLIDE
            lower, upper = vec([lim["lower"], lim["upper"]])
            error = travel - min(max(travel, lower), upper)
            info["slides"].append((k, as_float(travel), as_float(error)))
            for body in (a, b):
                info["slide_margin"][body] = min(info["slide_margin"][body], abs(as_float(travel - lower)), abs(as_float(travel - upper)))
            if error == 0:
                if mutation == "nonbinding_slide_counted":
                    ex_n[a] += 1
                    ex_n[b] += 1
                continue
            push(n_axis, error / (w_linear(n_axis) + compliance))
        pi = num.atan2(vec([1.0])[0], vec([1.0])[0]) * 4
        for index, drv in drives_of[k]:                                     # 3. the drives, in the caller's order
            kind = int(drv["kind"])
            target, alpha, max_force = vec([drv["target"], drv["compliance"], drv["max_force"]])
            at_start = integrated if mutation == "velocity_from_integrated" else past
            angular_kind = kind in (DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY)
            if angular_kind:
                measure = hinge_phi(e_rot, a, b, jt["axis_a"], drv["ref_a"], drv["ref_b"])
                if kind == DRIVE_ANGLE:
                    x = measure - target
                else:
                    x = measure - hinge_phi(at_start[1], a, b, jt["axis_a"], drv["ref_a"], drv["ref_b"])
                wrapped = x if mutation == "wrap_dropped" else (x - pi * 2 if x > pi else (x + pi * 2 if x < -pi else x))
                error = wrapped if kind == DRIVE_ANGLE else wrapped - target * h
                margin = abs(np.pi - abs(as_float(x)))                   # x lies in (-2 pi, 2 pi): the jumps are at +-pi
                for body in (a, b):
                    info["drive_wrap_margin"][body] = min(info["drive_wrap_margin"][body], margin)
                w = w_angular(n_axis)
            else:
                measure = travel
                if kind == DRIVE_POSITION:
                    error = travel - target
                else:
                    assert kind == DRIVE_VELOCITY
                    p0, _ = anchors(at_start[0], at_start[1], jt)
                    error = (travel - dot(p0[1] - p0[0], qrot(at_start[1][:, a], vec(jt["axis_a"])))) - target * h
                w = w_linear(n_axis, angular_half=mutation != "linear_drive_w_without_angular")
            for body in (a, b):
                info["drive_margin"][body] = min(info["drive_margin"][body], abs(as_float(error)))
            if error == 0:
                info["drives"].append((index, kind, 0.0, False, as_float(measure)))
                continue
            base = alpha if mutation == "drive_without_base_compliance" else alpha + vec([1e-6])[0]
            lam = error / (w + base / (h * h))
            cap = max_force * (h if mutation == "clamp_by_h" else h * h)
            clamped = bool(lam > cap or lam < -cap)
            lam = min(max(lam, -cap), cap)
            info["drives"].append((index, kind, as_float(error), clamped, as_float(measure)))
            counted = not (clamped and mutation == "clamped_uncounted")
            if clamped:
                info["n_clamped"][[a, b]] += 1
            if angular_kind:
                extra(a, None, matvec(inertia(a), n_axis * lam), counted)
                extra(b, None, matvec(inertia(b), n_axis * (lam if mutation == "angular_drive_same_sign" else -lam)), counted)
            else:
                push(n_axis, lam, counted)
        for body in (a, b):                                                 # ... and added after the joint's other entries
            if ex_n[body] or ex_entries[body]:
                sum_p[:, body] = sum_p[:, body] + ex_p[body]
                sum_q[:, body] = sum_q[:, body] + ex_q[body]
                count[body] += 0 if mutation in ("extras_uncounted", "joints_uncounted") else ex_n[body]
                info["n_extra"][body] += ex_entries[body]
                info["n_joint"][body] += ex_entries[body]
    return sum_p, sum_q, count, info


def _scalars(num, x):
    x = np.asarray(x)
    return num.conv(x) if x.dtype == np.float64 else x


def bounce(num, s, pose, velocities, start_velocities, manifolds, mask, vert, h, restitution, ground_restitution,
           bounce_threshold, terrain=None, mutation=None, integrated=None, ground_xs=None, compliance=None):
    """Stage 6: include/xpbd.h, "RESTITUTION", and the restitution paragraph of "TERRAIN", written from that prose alone; it
    follows neither tests/restitution_model.py, tests/terrain_model.py, xpbd_step.hpp nor the kernels.  pose = (x, q) after
    derive, velocities = (v, w) after derive, start_velocities = (v0, w0) before integrate, all (3 | 4, n) model scalars;
    manifolds and mask: THIS substep's, formed at the post-integrate poses; restitution: f64 per body or None (all 0).
      e        the header's compare-and-select, (e_inc < e_ref) ? e_ref : e_inc; ground: (e_b < e_ground) ? e_ground : e_b.
      manifold XPBD_RESTITUTION_SWEEPS passes over its points in point order on copies of the two bodies' post-derive
               velocities; a visit does nothing unless e > 0 && vn0 < -bounce_threshold && Wsum > 0; wanted = total_k +
               ((-e) vn0 - vn) / Wsum, no compliance; if (!(wanted > 0)) wanted = 0; lambda = wanted - total_k, nothing
               more when it is 0; +lambda n on the incident copy at p_inc, -lambda n on the reference copy at p_ref, at once.
               n: stage N's reference plane normal of a face contact, d / |d| with d = p_ref - p_inc of the one-point
               contact (no visit at |d| == 0).  A manifold in which no visit applied an impulse makes no entry.
      Jacobi   every body adds the entries (v_copy - v, w_copy - w) of its manifolds in neighbour order from 0 and applies
               sum / count.
      ground   then, per body, the set bits of the mask in ascending vertex order, sequentially on the body's current v, w:
               p = Rigid::frame() at (x, q) * vertex, n = (0, 0, 1) or -- with a terrain -- the plane's normal of the lookup
               repeated at p (outside: no entry); entry iff e > 0 && vn0 < -bounce_threshold && Wsum > 0 && vn < (-e) vn0.
    Arms and W are formed at (x, q): arm = p - (x + center_of_mass), W = inverse_mass + (I^-1 a) . a, a = q^-1 (arm x n); an
    impulse P changes v by P inverse_mass and w by (I^-1 arm) x P, the arm NOT rotated into rest space (rigid.rs:113-123).
    Poses are not touched.
    Continuity.  The clamp !(wanted > 0) and the ground condition vn < (-e) vn0 are continuous: lambda is 0 at the boundary,
    so which side a rounding takes changes nothing, and neither excludes a body.  The threshold vn0 < -bounce_threshold is
    a jump (threshold_margin), and so is a manifold's entry: with no applied impulse its count of 1 vanishes (entry_margin).
    Returns (v, w, info); info per body: bounce_pair_entries, bounce_one_point (those of them from a manifold of one point),
    bounce_ground_entries, bounce_push / bounce_give_back /
    bounce_clamped (visits with lambda > 0, lambda < 0, wanted clamped to 0), threshold_margin (smallest |vn0 + threshold| h of
    a point with e > 0 and Wsum > 0: metres), entry_margin (metres: of a manifold that takes part and applies nothing the
    smallest |(-e) vn0 - vn| h of its visits; of one that has an entry the largest |lambda| Wsum h), bounce_cell_margin,
    bounce_diagonal_margin, bounce_border_margin (the repeated terrain lookup's), `bounce_seen`, a set of tags, and
    `bounce_impulses`, every point's total impulse after the last pass and every ground entry's lambda (f64)."""
    assert mutation is None or mutation in BOUNCE_MUTATIONS
    sqrt = num.sqrt
    im, M, com = s["inverse_mass"], s["inverse_inertia"], s["center_of_mass"]
    pos, rot = pose
    vel, ang = velocities
    v0, w0 = (vel, ang) if mutation == "vn0_post_derive" else start_velocities
    a_pos, a_rot = integrated if mutation == "arms_at_integrated" else (pos, rot)
    n = pos.shape[1]
    e_body = np.zeros(n) if restitution is None else np.asarray(restitution, dtype=np.float64)
    threshold = num.conv(np.array([float(bounce_threshold)]))[0]
    info = {k: np.zeros(n, dtype=np.int64) for k in ("bounce_pair_entries", "bounce_ground_entries", "bounce_push",
                                                     "bounce_give_back", "bounce_clamped", "bounce_one_point")}
    info.update({k: np.full(n, np.inf) for k in ("threshold_margin", "entry_margin", "bounce_cell_margin",
                                                 "bounce_diagonal_margin", "bounce_border_margin")})
    seen = set()
    impulses = []                                                        # every point's final total and every ground lambda
    lookup_mutation = mutation if mutation in xm.TERRAIN_MUTATIONS else None

    def as_float(x):
        return float(num.to_f64(np.array([x]))[0])

    def lower(key, bodies, value):
        for b in bodies:
            info[key][b] = min(info[key][b], value)

    def arm_of(b, p):
        return p - (a_pos[:, b] + com[:, b])

    def resistance(b, arm, normal):
        a = qrot(conj(a_rot[:, b]), cross(arm, normal))
        return im[b] + dot(matvec(M[:, :, b], a), a)

    def push(b, v, w, arm, impulse):
        lever = qrot(conj(a_rot[:, b]), arm) if mutation == "impulse_arm_in_rest_space" else arm
        return v + impulse * im[b], w + cross(matvec(M[:, :, b], lever), impulse)

    def pairs(vel, ang):
        entries = [[] for _ in range(n)]
        for (i, j), m in sorted(manifolds.items()):
            if m["separated"] or not len(m["p_ref"]):
                continue
            ref, inc = (j, i) if m["feature"] == FACE_B else (i, j)
            e_inc, e_ref = float(e_body[inc]), float(e_body[ref])
            e64 = (e_ref if e_inc < e_ref else e_inc) if mutation != "e_smaller_side" else min(e_inc, e_ref)
            if e_inc != e_ref and e64 > 0:
                seen.add("larger e on the incident side" if e_inc > e_ref else "larger e on the reference side")
            e = num.conv(np.array([e64]))[0]
            points = []
            for p_ref, p_inc in zip(m["p_ref"], m["p_inc"]):
                p_ref, p_inc = _scalars(num, p_ref), _scalars(num, p_inc)
                if m["feature"] == EDGES:
                    d = p_ref - p_inc
                    length = sqrt(dot(d, d))
                    if length == 0:
                        continue
                    normal = d / length
                else:
                    normal = _scalars(num, m["normal"])
                arm_i, arm_r = arm_of(inc, p_inc), arm_of(ref, p_ref)
                w_sum = resistance(inc, arm_i, normal) + resistance(ref, arm_r, normal)
                if mutation == "compliance_in_wsum":
                    w_sum = w_sum + compliance
                vn0 = dot(normal, (v0[:, inc] + cross(w0[:, inc], arm_i)) - (v0[:, ref] + cross(w0[:, ref], arm_r)))
                points.append((normal, arm_i, arm_r, w_sum, vn0))
                if e64 > 0 and w_sum > 0:
                    lower("threshold_margin", (inc, ref), abs(as_float(vn0 + threshold) * h))
                    seen.add("a point over the threshold" if vn0 < -threshold else "a point under the threshold")
            copies = {inc: (vel[:, inc], ang[:, inc]), ref: (vel[:, ref], ang[:, ref])}
            totals = [e * 0 for _ in points]
            applied, idle_gap, largest = False, np.inf, 0.0

            def closing(normal, arm_i, arm_r):
                (vi, wi), (vr, wr) = copies[inc], copies[ref]
                return dot(normal, (vi + cross(wi, arm_i)) - (vr + cross(wr, arm_r)))

            def takes_part(w_sum, vn, vn0):
                tested = vn if mutation == "threshold_on_vn" else vn0
                return e64 > 0 and bool(tested < -threshold) and bool(w_sum > 0)

            if mutation == "points_averaged":            # every point from the same copies, a share of 1 / points each
                lams = []
                for normal, arm_i, arm_r, w_sum, vn0 in points:
                    vn = closing(normal, arm_i, arm_r)
                    lam = ((-e) * vn0 - vn) / w_sum if takes_part(w_sum, vn, vn0) else e * 0
                    lams.append(lam / len(points) if lam > 0 else e * 0)
                for lam, (normal, arm_i, arm_r, _, _) in zip(lams, points):
                    if lam != 0:
                        applied = True
                        copies[inc] = push(inc, *copies[inc], arm_i, normal * lam)
                        copies[ref] = push(ref, *copies[ref], arm_r, normal * -lam)
            else:
                for _ in range(1 if mutation == "one_sweep" else SWEEPS):
                    for k, (normal, arm_i, arm_r, w_sum, vn0) in enumerate(points):
                        vn = closing(normal, arm_i, arm_r)
                        if not takes_part(w_sum, vn, vn0):
                            continue
                        step = ((-e) * vn0 - vn) / w_sum
                        wanted = totals[k] + step
                        clamped = not bool(wanted > 0)
                        if clamped:
                            wanted = wanted * 0
                        if mutation == "no_give_back":     # lambda clamped, not the total
                            wanted = totals[k] + (step if step > 0 else step * 0)
                        lam = wanted - totals[k]
                        info["bounce_clamped"][[inc, ref]] += 1 if clamped else 0
                        if lam == 0:
                            idle_gap = min(idle_gap, abs(as_float((-e) * vn0 - vn)) * h)
                            continue
                        totals[k] = wanted
                        applied = True
                        largest = max(largest, abs(as_float(lam * w_sum)) * h)
                        info["bounce_push" if lam > 0 else "bounce_give_back"][[inc, ref]] += 1
                        copies[inc] = push(inc, *copies[inc], arm_i, normal * lam)
                        copies[ref] = push(ref, *copies[ref], arm_r, normal * (lam if mutation == "reference_pushed_same_way" else -lam))
            impulses.extend(as_float(x) for x in totals)
            if applied:
                lower("entry_margin", (inc, ref), largest if mutation != "points_averaged" else np.inf)
            elif idle_gap < np.inf:
                lower("entry_margin", (inc, ref), idle_gap)
                seen.add("a manifold that takes part without an entry")
            if applied or (mutation == "idle_counted" and points):
                for b in (inc, ref):
                    entries[b].append((copies[b][0] - vel[:, b], copies[b][1] - ang[:, b]))
                    info["bounce_pair_entries"][b] += 1
                    info["bounce_one_point"][b] += len(points) == 1
        vel, ang = vel.copy(), ang.copy()
        for b in range(n):
            if entries[b]:
                dv, dw = vel[:, b] * 0, ang[:, b] * 0
                for x, y in entries[b]:
                    dv, dw = dv + x, dw + y
                count = 1 if mutation == "entries_summed" else len(entries[b])
                vel[:, b], ang[:, b] = vel[:, b] + dv / count, ang[:, b] + dw / count
        return vel, ang

    def grounded(vel, ang):
        vel, ang = vel.copy(), ang.copy()
        up = num.conv(np.array([0.0, 0.0, 1.0]))
        for b in np.nonzero(mask)[0]:
            e_b = float(e_body[b])
            e64 = (ground_restitution if e_b < ground_restitution else e_b) if mutation != "e_smaller_side" else min(e_b, ground_restitution)
            e = num.conv(np.array([e64]))[0]
            frame_p = a_pos[:, b] + com[:, b] + qrot(a_rot[:, b], -com[:, b])        # Rigid::frame, rigid.rs:75-80
            v, w = vel[:, b], ang[:, b]
            before = (v, w)
            for k in range(len(vert)):
                if not (int(mask[b]) >> k) & 1:
                    continue
                p = frame_apply(frame_p, a_rot[:, b], vert[k][:, b])
                normal = up
                if terrain is not None:
                    at = ground_xs[k][:, b] if mutation == "bounce_lookup_at_integrated" else p
                    inside, pn, _, where = xm.terrain_lookup(num, terrain, at[:, None], lookup_mutation)
                    for key in ("cell", "diagonal", "border"):
                        lower("bounce_%s_margin" % key, (b,), float(where[key][0]))
                    if not inside[0]:
                        seen.add("a bounce vertex outside the field")
                        continue
                    if mutation != "bounce_normal_vertical":
                        normal = pn[:, 0]
                arm = arm_of(b, p)
                w_sum = resistance(b, arm, normal)
                if mutation == "compliance_in_wsum":
                    w_sum = w_sum + compliance
                rv, rw = before if mutation == "ground_reads_pre_ground" else (v, w)
                vn = dot(normal, rv + cross(rw, arm))
                vn0 = dot(normal, v0[:, b] + cross(w0[:, b], arm))
                if not (e64 > 0 and bool(w_sum > 0)):
                    continue
                lower("threshold_margin", (b,), abs(as_float(vn0 + threshold) * h))
                tested = vn if mutation == "threshold_on_vn" else vn0
                seen.add("a point over the threshold" if vn0 < -threshold else "a point under the threshold")
                if not (bool(tested < -threshold) and bool(vn < (-e) * vn0)):
                    continue
                lam = ((-e) * vn0 - vn) / w_sum
                v, w = push(b, v, w, arm, normal * lam)
                impulses.append(as_float(lam))
                info["bounce_ground_entries"][b] += 1
                if terrain is not None:
                    seen.add("a terrain bounce")
            vel[:, b], ang[:, b] = v, w
        return vel, ang

    if mutation == "ground_before_pairs":
        vel, ang = pairs(*grounded(vel, ang))
    else:
        vel, ang = grounded(*pairs(vel, ang))
    if info["bounce_pair_entries"].any():
        seen.add("a pair entry")
    if info["bounce_ground_entries"].any():
        seen.add("a ground entry")
    for key, tag in (("bounce_push", "a pushing visit"), ("bounce_give_back", "a give-back visit"), ("bounce_clamped", "a clamped wanted")):
        if info[key].any():
            seen.add(tag)
    info["bounce_seen"] = seen
    info["bounce_impulses"] = np.array(impulses)
    return vel, ang, info


def is_fixed(s):
    """FIXED (xpbd.h, the islands' definition): inverse_mass and all nine inverse_inertia entries == 0.  (n,) bool."""
    zero = np.array([bool(x == 0) for x in s["inverse_mass"]])
    M = s["inverse_inertia"]
    for c in range(3):
        for r in range(3):
            zero &= np.array([bool(x == 0) for x in M[c, r]])
    return zero


def kinematic_velocities(num, s, pos, rot, entries, h, r, mutation=None, substep_index=0):
    """Stage 0: include/xpbd.h, "KINEMATIC bodies", the overwrite before the integrate stage of a substep with `r` substeps
    left, written from that prose alone.  pos, rot: (3, n), (4, n) model scalars, the bodies' position and rotation FIELDS (what
    a download shows, not Rigid::frame()); entries: records with the fields of xpbd_kinematic; h in model scalars.
      POSE      velocity = (p_t - p) / (r h);  dq = q_t * conjugate(q), negated if dq.s < 0;  m = |vec(dq)|;  m == 0: angular
                velocity 0;  else half = atan2(m, dq.s), angular velocity = vec(dq) * ((2 / h) * tan(half / r) / m).
      VELOCITY  velocity = linear, angular velocity = angular[0..2], before every substep.
    Returns ({body: (velocity (3,), angular velocity (3,))}, info); info per body (inf / False without an entry):
    kin_flip_margin |dq.s| (the negation jumps at 0), kin_tan_margin |pi / 2 - half / r| (tan's pole; half / r <= pi / 2 always,
    with equality only at r = 1 and dq.s == 0) and kin_zero (m == 0), and kin_mode (-1 without an entry).
    substep_index: k, read by two of the wrong readings only (`r` counted as k + 1; VELOCITY asserted at k == 0 only)."""
    assert mutation is None or mutation in KINEMATIC_MUTATIONS
    n = pos.shape[1]
    com = s["center_of_mass"]
    info = {"kin_flip_margin": np.full(n, np.inf), "kin_tan_margin": np.full(n, np.inf), "kin_zero": np.zeros(n, dtype=bool),
            "kin_mode": np.full(n, -1, dtype=np.int64), "kin_negated": np.zeros(n, dtype=bool)}
    out = {}
    one = h * 0 + 1
    left = substep_index + 1 if mutation == "r_counted_up" else r
    pi = num.atan2(one, one) * 4
    for e in entries:
        b, mode = int(e["body"]), int(e["mode"])
        info["kin_mode"][b] = mode
        linear = num.conv(np.asarray(e["linear"], dtype=np.float64))
        angular = num.conv(np.asarray(e["angular"], dtype=np.float64))
        if mode == 1:                                                        # XPBD_KINEMATIC_VELOCITY
            if mutation == "velocity_once_per_frame" and substep_index > 0:
                continue
            out[b] = (linear, angular[:3])
            continue
        assert mode == 0                                                     # XPBD_KINEMATIC_POSE
        p, q = pos[:, b], rot[:, b]
        if mutation == "p_frame_origin":
            p = p + com[:, b] + qrot(q, -com[:, b])
        v = (linear - p) / (h * left)
        dq = qmul(conj(q), angular) if mutation == "dq_conjugate_first" else qmul(angular, conj(q))
        info["kin_flip_margin"][b] = abs(float(num.to_f64(np.array([dq[0]]))[0]))
        if dq[0] < 0 and mutation != "dq_not_negated":
            dq = -dq
            info["kin_negated"][b] = True
        m = num.sqrt(dot(dq[1:], dq[1:]))
        if m == 0:
            info["kin_zero"][b] = True
            out[b] = (v, dq[1:] * 0)
            continue
        half = num.atan2(m, dq[0])
        if mutation == "full_angle":
            half = half * 2
        info["kin_tan_margin"][b] = abs(float(num.to_f64(np.array([pi / 2 - half / left]))[0]))
        out[b] = (v, dq[1:] * ((one * 2 / h) * num.tan(half / left) / m))
    return out, info


def damp(num, s, pose, velocities, joints, rows, joint_damping, h, mutation=None, integrated=None):
    """Stage 7: include/xpbd.h, "DAMPING", steps 1 to 3, written from that prose alone.  pose = (x, q), velocities = (v, w):
    (3 | 4, n) model scalars as stage 6 left them (derive's with stage 6 off); joints: records of xpbd_joint; rows: records of
    xpbd_body_damping, one per body, or None (every row the default); joint_damping: records of xpbd_joint_damping or None; h in
    model scalars.  A FIXED body keeps its velocities; nothing else is touched.
      1. dampers  Jacobi: every term of every joint is evaluated on (x, q, v, w) of ALL bodies as given; joints in ascending
                  index.  c = x + center_of_mass, p_a, p_b = Rigid::frame() at (x, q) times the anchor, k = mu h < 1 ? mu h : 1.
                  linear (mu_l > 0): d = u_b(p_b) - u_a(p_a), u(p) = v + w x (p - c); len = |d|, no term at 0; n = d (1 / len);
                  Wsum = W_a(p_a, n) + W_b(p_b, n), W = inverse_mass + (I^-1 a) . a, a = q^-1 ((p - c) x n); no term unless
                  Wsum > 0; lambda = k len / Wsum; +lambda n at p_a on a, -lambda n at p_b on b: dv = P inverse_mass,
                  dw = (I^-1 (p - c)) x P.  angular (mu_a > 0), on the SAME velocities: d = w_b - w_a, n = d (1 / len),
                  Wang = (I_a^-1 n_a) . n_a + (I_b^-1 n_b) . n_b, n_a = q_a^-1 n; lambda = k len / Wang; a turns by
                  q_a (I_a^-1 (q_a^-1 (lambda n))), b by the same with -lambda.  A joint's entry for a body is the sum of its
                  terms' changes, the linear one first; no term, no entry.  v += sum of entries / number of entries.
      2. drag     v = v * (1 / (1 + h c_l)), w likewise with c_a.
      3. caps     m = |v|; if m > cap: v = v * (cap / m); likewise w.
    Continuity.  The clamp of k and drag are continuous, and Wsum > 0 fails only where both ends are fixed, exactly: none changes
    anything discretely.  A cap that fires scales by cap / m, which is 1 at the boundary: continuous, but the cases file takes
    cap_margin in (0, TAU] out all the same; a term's direction d / len is not continuous at len == 0 (damper_cond).
    Returns (v, w, info); info per body: n_damper_entries, n_damper_terms, damper_cond (smallest len h of a term of one of its
    joints, metres or radians; inf without), cap_margin (smallest |m - cap| h over its two caps; inf for +inf), cap_fired_linear,
    cap_fired_angular, n_damper_fixed_end (its entries from a joint whose other end is fixed), the set `damping_seen` and the
    list `damper_terms` of (joint, "linear" | "angular", k, len) in f64."""
    assert mutation is None or mutation in DAMPING_MUTATIONS
    sqrt = num.sqrt
    im, M, com = s["inverse_mass"], s["inverse_inertia"], s["center_of_mass"]
    pos, rot = pose
    vel, ang = velocities
    a_pos, a_rot = integrated if mutation == "anchors_at_integrated" else (pos, rot)
    n = pos.shape[1]
    fixed = is_fixed(s)
    one = h * 0 + 1
    info = {"n_damper_entries": np.zeros(n, dtype=np.int64), "n_damper_terms": np.zeros(n, dtype=np.int64),
            "damper_cond": np.full(n, np.inf), "cap_margin": np.full(n, np.inf), "cap_fired_linear": np.zeros(n, dtype=bool),
            "cap_fired_angular": np.zeros(n, dtype=bool), "n_damper_fixed_end": np.zeros(n, dtype=np.int64)}
    seen = set()
    terms_of = {}

    def as_float(x):
        return float(num.to_f64(np.array([x]))[0])

    def const(x):
        return num.conv(np.array([float(x)]))[0]

    coefficient = {}
    for d in ([] if joint_damping is None else joint_damping):
        coefficient[int(d["joint"])] = (float(d["linear"]), float(d["angular"]))

    def share(mu):
        k = const(mu) * h
        if mutation == "k_unclamped":
            return k
        return k if k < 1 else one

    def centre(b):
        return a_pos[:, b] if mutation == "damper_arm_without_com" else a_pos[:, b] + com[:, b]

    def anchor(b, local):
        frame_p = a_pos[:, b] + com[:, b] + qrot(a_rot[:, b], -com[:, b])            # Rigid::frame()
        return frame_apply(frame_p, a_rot[:, b], num.conv(np.asarray(local, dtype=np.float64)))

    def joint_entries(j, jt, v, w):
        """The two ends' entries ((dv, dw) or None, terms) of joint j on the velocities (v, w)."""
        mu_l, mu_a = coefficient.get(j, (0.0, 0.0))
        a, b = int(jt["body_a"]), int(jt["body_b"])
        dv = {a: vel[:, 0] * 0, b: vel[:, 0] * 0}
        dw = {a: vel[:, 0] * 0, b: vel[:, 0] * 0}
        terms, kinds = 0, []
        if mu_l == 0 and mu_a == 0:
            return a, b, None, 0, kinds
        wa, wb = w[:, a], w[:, b]
        if mu_l > 0:
            p_a, p_b = anchor(a, jt["anchor_a"]), anchor(b, jt["anchor_b"])
            arm_a, arm_b = p_a - centre(a), p_b - centre(b)
            d = (v[:, b] + cross(wb, arm_b)) - (v[:, a] + cross(wa, arm_a))
            length = sqrt(dot(d, d))
            if length != 0:
                for body in (a, b):
                    info["damper_cond"][body] = min(info["damper_cond"][body], as_float(length * h))
                nrm = d * (one / length)
                w_sum = 0
                for body, arm in ((a, arm_a), (b, arm_b)):
                    local = qrot(conj(a_rot[:, body]), cross(arm, nrm))
                    w_sum = w_sum + (im[body] + dot(matvec(M[:, :, body], local), local))
                if w_sum > 0:
                    seen.add("mu_l h below 1" if const(mu_l) * h < 1 else "mu_l h at or above 1")
                    lam = (share(mu_l) * length) / w_sum
                    terms_of[(j, "linear")] = (as_float(share(mu_l)), as_float(length))
                    for body, arm, P in ((a, arm_a, nrm * lam), (b, arm_b, nrm * (lam if mutation == "second_end_same_sign" else -lam))):
                        dv[body] = dv[body] + P * im[body]
                        dw[body] = dw[body] + cross(matvec(M[:, :, body], arm), P)
                    terms += 1
                    kinds.append("linear")
                    if mutation == "angular_on_linear_result":
                        wa, wb = wa + dw[a], wb + dw[b]
        if mu_a > 0:
            d = wb - wa
            length = sqrt(dot(d, d))
            if length != 0:
                for body in (a, b):
                    info["damper_cond"][body] = min(info["damper_cond"][body], as_float(length * h))
                nrm = d * (one / length)
                local = {body: (nrm if mutation == "wang_unrotated" else qrot(conj(a_rot[:, body]), nrm)) for body in (a, b)}
                w_ang = dot(matvec(M[:, :, a], local[a]), local[a]) + dot(matvec(M[:, :, b], local[b]), local[b])
                if w_ang > 0:
                    seen.add("mu_a h below 1" if const(mu_a) * h < 1 else "mu_a h at or above 1")
                    lam = (share(mu_a) * length) / w_ang
                    terms_of[(j, "angular")] = (as_float(share(mu_a)), as_float(length))
                    for body, signed in ((a, lam), (b, -lam)):
                        turn = qrot(conj(a_rot[:, body]), nrm * signed)
                        dw[body] = dw[body] + qrot(a_rot[:, body], matvec(M[:, :, body], turn))
                    terms += 1
                    kinds.append("angular")
        if not terms:
            return a, b, None, 0, kinds
        return a, b, {a: (dv[a], dw[a]), b: (dv[b], dw[b])}, terms, kinds

    def dampers(vel, ang):
        sequential = mutation == "neighbour_stage7_velocities"
        out_v, out_w = vel.copy(), ang.copy()
        read_v, read_w = (out_v, out_w) if sequential else (vel, ang)
        for body in range(n):
            sum_v, sum_w, entries, terms = vel[:, body] * 0, vel[:, body] * 0, 0, 0
            for j, jt in enumerate(joints):
                if body not in (int(jt["body_a"]), int(jt["body_b"])):
                    continue
                a, b, entry, t, kinds = joint_entries(j, jt, read_v, read_w)
                if entry is None:
                    continue
                sum_v, sum_w = sum_v + entry[body][0], sum_w + entry[body][1]
                entries, terms = entries + 1, terms + t
                other = b if body == a else a
                if not fixed[body]:
                    seen.add({("linear",): "a linear-only entry", ("angular",): "an angular-only entry",
                              ("linear", "angular"): "a two-term entry"}[tuple(kinds)])
                    if fixed[other]:
                        info["n_damper_fixed_end"][body] += 1
                        seen.add("a damper with one end fixed")
            info["n_damper_entries"][body], info["n_damper_terms"][body] = entries, terms
            if entries and (not fixed[body] or mutation == "fixed_body_damped"):
                count = {"count_is_terms": terms, "damper_entries_summed": 1}.get(mutation, entries)
                out_v[:, body] = read_v[:, body] + sum_v / count
                out_w[:, body] = read_w[:, body] + sum_w / count
        for jt in joints:
            a, b = int(jt["body_a"]), int(jt["body_b"])
            ea, eb = info["n_damper_entries"][a], info["n_damper_entries"][b]
            if ea and eb and ea != eb and not fixed[a] and not fixed[b]:
                seen.add("ends with unequal counts")
        return out_v, out_w

    def row(b):
        if rows is None:
            return 0.0, 0.0, np.inf, np.inf
        r = rows[b]
        return float(r["linear"]), float(r["angular"]), float(r["max_linear_speed"]), float(r["max_angular_speed"])

    def moved(b):
        return not fixed[b] or mutation == "fixed_body_damped"

    def drag(vel, ang):
        vel, ang = vel.copy(), ang.copy()
        for b in range(n):
            if not moved(b):
                continue
            c_l, c_a = row(b)[:2]
            for arr, c in ((vel, c_l), (ang, c_a)):
                scale = one - h * const(c) if mutation == "drag_explicit" else one / (one + h * const(c))
                arr[:, b] = arr[:, b] * scale
        return vel, ang

    def caps(vel, ang):
        vel, ang = vel.copy(), ang.copy()
        for b in range(n):
            if not moved(b):
                continue
            for arr, cap, key in ((vel, row(b)[2], "cap_fired_linear"), (ang, row(b)[3], "cap_fired_angular")):
                if not np.isfinite(cap):
                    continue
                c = const(cap)
                if mutation == "cap_per_component":
                    arr[:, b] = np.array([min(max(x, -c), c) for x in arr[:, b]], dtype=arr.dtype)
                    continue
                m = sqrt(dot(arr[:, b], arr[:, b]))
                info["cap_margin"][b] = min(info["cap_margin"][b], abs(as_float(m - c)) * as_float(h))
                if m > c:
                    arr[:, b] = arr[:, b] * (c / m)
                    info[key][b] = True
                seen.add(("%s cap that fires" if m > c else "%s cap that does not fire") % ("a linear" if arr is vel else "an angular"))
        return vel, ang

    order = {"caps_before_drag": (dampers, caps, drag), "drag_before_dampers": (drag, dampers, caps)}.get(mutation, (dampers, drag, caps))
    for stage in order:
        vel, ang = stage(vel, ang)
    info["damping_seen"] = seen
    info["damper_terms"] = [(j, kind, k, length) for (j, kind), (k, length) in sorted(terms_of.items())]
    return vel, ang, info


def substep(bodies, shapes, shape_id, h, manifolds=None, mu=None, ground_mu=np.inf, max_depenetration_speed=0.0, num=None,
            mutation=None, tau=0.0, joints=(), limits=(), drives=(), restitution=None, ground_restitution=0.0,
            bounce_threshold=0.0, terrain=None, kinematics=None, substeps_left=1, damping=None, joint_damping=None,
            substep_index=0, asleep=None, contact_mask=None):
    """Stage S: one contacts substep (steps 1, 3, 4, 5 of xpbd_pairs_oracle.h) of n bodies ((n, 38) f64).  shapes: list of
    shape() dicts.  manifolds: {(i, j), i < j: {"feature", "p_ref": [(3,)], "p_inc": [(3,)]}} of the touching pairs at the
    post-integrate frames, or None: stage N on every pair (stage S o N, the fully independent substep).  mu: per-body
    friction coefficients (None: the reference's contact), ground_mu the plane's.  mutation: one of MUTATIONS, a
    deliberately wrong reading for the mutation check (MUTATIONS, or JOINT_MUTATIONS for the joint entries).  joints, limits:
    records with the fields of xpbd_joint / xpbd_joint_limit: all their entries are evaluated on the poses after step 3, in
    the same Jacobi pass as the pair points, and a body applies the average of ALL its entries -- pair points, positional
    joint entries, hinge entries and binding limits each count 1 (joint_terms).  Friction and the depenetration limit never
    touch a joint entry.  drives: records of xpbd_joint_drive; a joint's extra entries (SLIDER, XPBD_LIMIT_SLIDE, drives) are
    read at the same poses, the velocity drives' subscript-0 quantities at the poses the substep started from, and each
    counts 1 in the same average (joint_terms).  restitution (f64 per body, or None), ground_restitution, bounce_threshold:
    stage 6, the velocity pass of xpbd.h's "RESTITUTION", after derive (bounce); with restitution None and ground_restitution
    0 the stage is not run.  terrain (xprec_model.heightfield): the ground of step 3 and of stage 6's ground part in place of
    the plane z = 0 (xprec_model.ground, xprec_model.terrain_lookup).  Without the four the result is what it was.

    Returns a dict: state (n, 38) model scalars; frames: the post-integrate frames [(position, rotation)]; manifolds: the
    ones used; per body: mask, margin, cond, flip_margin, domain (as xprec_model.step), branch (smallest distance in
    metres of a friction or depenetration-limit comparison from its threshold) and pair_cond (smallest |c1 - c0| of a
    pair point); undecided: the pairs whose stage N manifold has a margin in (0, tau]; n_points (pair-contact points of the
    body) and, from joint_terms, n_joint, n_binding, limit_margin, wrap_margin, joint_cond, `limits` and the extras' n_extra,
    n_clamped, slide_margin, drive_margin, drive_wrap_margin, `slides`, `perps`, `drives`; from xprec_model.ground cell_margin,
    diagonal_margin, border_margin, lower_contacts, upper_contacts, n_outside (inf and 0 without a terrain; `margin` is then
    min |s|); and, when stage 6 ran, bounce's info.
    kinematics (records of xpbd_kinematic) and substeps_left (r): stage 0, kinematic_velocities, overwrites the entries' two
    velocities before integrate; stage 6 reads them as v0, w0.  damping (records of xpbd_body_damping, one per body) and
    joint_damping (records of xpbd_joint_damping): stage 7, damp, after stage 6 -- after derive with stage 6 off.  Without the
    four the result is what it was; with them the stages' info is in the dict too.  substep_index: see kinematic_velocities.
    asleep ((n,) bool, or None: nobody, and the result is what it was): xpbd.h, "SLEEPING", rules (a)-(c), written from that
    section alone; xpbd_sleep.hip, xpbd_contacts.hip, xpbd_restitution.hip, xpbd_world_sleep.cpp and sleep_model.py were not read
    for it.  An asleep body has no stage: no overwrite, integrate, ground contacts, derive, stage 6 or 7; its 13 dynamic values
    are returned as the input's bits and its contact mask as contact_mask's entry (0 without one).  Everybody else sees it through
    a record of its stored pose: P0 = P1 = Rigid::frame() of that pose (stage N, every pair point, friction's past frame), the pose
    after the ground contacts = that pose, its own inverse mass and inverse inertia in the shared denominator; its part of the
    correction is dropped and counted nowhere, stage 6 reads its start and post-derive velocities as zero and drops its entry, and a
    pair of two inert (asleep or FIXED) bodies does not exist.  Info: n_sleeper_points, per body the pair points whose other end
    is asleep, and `asleep`."""
    assert mutation is None or mutation in (MUTATIONS + JOINT_MUTATIONS + DRIVE_MUTATIONS + BOUNCE_MUTATIONS + DAMPING_MUTATIONS
                                            + KINEMATIC_MUTATIONS + SLEEP_MUTATIONS)
    sleep_mutation = mutation if mutation in SLEEP_MUTATIONS else None
    joint_mutation = mutation if mutation in JOINT_MUTATIONS + DRIVE_MUTATIONS else None
    num = num or xm.native()
    sqrt = num.sqrt
    b64 = np.ascontiguousarray(bodies, dtype=np.float64).reshape(-1, 38)
    n = b64.shape[0]
    sid = np.asarray(shape_id, dtype=np.int64)
    s = xm._unpack(b64, num)
    im, M, com = s["inverse_mass"], s["inverse_inertia"], s["center_of_mass"]
    pos, rot, vel, ang = s["position"], s["rotation"], s["velocity"], s["angular_velocity"]
    hx = num.const(float(h))
    compliance = num.const("1e-6") / (hx * hx)                           # solver.rs:20
    limit = hx * num.const(float(max_depenetration_speed)) if max_depenetration_speed > 0 else None
    domain = np.ones(n, dtype=bool)
    vmax = max(len(shapes[k]["verts"]) for k in set(sid.tolist()))
    counts = np.array([len(shapes[k]["verts"]) for k in sid])
    slots = np.zeros((n, vmax, 3))
    for b in range(n):
        slots[b, :counts[b]] = shapes[sid[b]]["verts"]
    vert = [num.conv(slots[:, v].T) for v in range(vmax)]

    # 0. the kinematic overwrite, before integrate                          xpbd.h, "KINEMATIC bodies"
    kin_mutation = mutation if mutation in KINEMATIC_MUTATIONS else None
    kin_info = {}

    def overwritten(vel, ang, at_pos, at_rot):
        scripted, info = kinematic_velocities(num, s, at_pos, at_rot, kinematics, hx, substeps_left, kin_mutation, substep_index)
        vel, ang = vel.copy(), ang.copy()
        for b, (v, w) in scripted.items():
            vel[:, b], ang[:, b] = v, w
        return vel, ang, info

    sleeping = asleep is not None
    zz = np.asarray(asleep, dtype=bool) if sleeping else np.zeros(n, dtype=bool)
    assert zz.shape == (n,)
    stored = (pos, rot, vel, ang)

    def keep(new, old):
        """`new` with the sleepers' columns taken from `old`."""
        out = new.copy()
        out[..., zz] = old[..., zz]
        return out

    before_vel, before_ang = vel, ang
    if kinematics is not None and len(kinematics) and kin_mutation != "overwrite_after_integrate":
        vel, ang, kin_info = overwritten(vel, ang, pos, rot)

    # 1. past = pose; integrate; P1 = Rigid::frame()                        solver.rs:7-10
    past_pos, past_rot = pos, rot
    start_vel, start_ang = (before_vel, before_ang) if kin_mutation == "v0_before_overwrite" else (vel, ang)   # v0, w0 of stage 6
    past_p = pos + com + qrot(rot, -com)
    pos, rot, vel, ang = xm.integrate(s, pos, rot, vel, ang, hx, sqrt)
    if kinematics is not None and len(kinematics) and kin_mutation == "overwrite_after_integrate":
        vel, ang, kin_info = overwritten(vel, ang, pos, rot)
    if sleeping:                                                          # rules (b), (c): no stage, and the record of the stored pose
        if sleep_mutation != "record_from_integrated":
            pos, rot = keep(pos, stored[0]), keep(rot, stored[1])
        vel, ang = keep(vel, stored[2]), keep(ang, stored[3])
        start_vel, start_ang = keep(start_vel, start_vel * 0), keep(start_ang, start_ang * 0)
        if sleep_mutation == "stage6_reads_stored_velocity":
            start_vel, start_ang = keep(start_vel, stored[2]), keep(start_ang, stored[3])
    p1_p, p1_q = pos + com + qrot(rot, -com), rot
    if sleeping:
        if sleep_mutation == "record_without_com":
            p1_p = keep(p1_p, pos)
        past_pos, past_rot, past_p = keep(past_pos, pos), keep(past_rot, rot), keep(past_p, p1_p)   # P0 = P1
    inert = zz | is_fixed(s) if sleeping else zz
    frames = [(p1_p[:, b], p1_q[:, b]) for b in range(n)]

    # 2. manifolds of all pairs by brute force (stage N), unless given
    undecided = []
    if manifolds is None:
        manifolds = {}
        centre = np.array([num.to_f64(frame_apply(p1_p[:, b], p1_q[:, b], num.conv(shapes[sid[b]]["centroid"]))) for b in range(n)])
        for i in range(n):
            for j in range(i + 1, n):
                if inert[i] and inert[j]:                                  # rule (a)
                    continue
                reach = shapes[sid[i]]["radius"] + shapes[sid[j]]["radius"]
                if np.linalg.norm(centre[i] - centre[j]) > reach + 1e-3:   # the bounding spheres are a millimetre apart
                    continue
                m = manifold(frames[i], frames[j], shapes[sid[i]], shapes[sid[j]], num)
                if not decided(m, tau):
                    undecided.append((i, j))
                if not m["separated"]:
                    manifolds[(i, j)] = m

    elif sleeping:
        manifolds = {k: m for k, m in manifolds.items() if not (inert[k[0]] and inert[k[1]])}

    # 3. ground contacts from P1, sequentially per body                     solver.rs:12-13
    body_mu = None
    if mu is not None or np.isfinite(ground_mu):
        body_mu = np.minimum(np.full(n, np.inf) if mu is None else np.asarray(mu, dtype=np.float64), ground_mu)
    integrated_pos, integrated_rot = pos, rot
    pos, rot, g = xm.ground(num, s, pos, rot, past_p, past_rot, vert, counts, compliance, domain, body_mu, limit, terrain,
                            mutation if mutation in xm.TERRAIN_MUTATIONS else None)
    if sleeping:
        if sleep_mutation != "record_after_ground":
            pos, rot = keep(pos, integrated_pos), keep(rot, integrated_rot)
        domain[zz] = True
        g["mask"][zz] = 0
        for key in ("margin", "cond", "branch", "cell_margin", "diagonal_margin", "border_margin"):
            g[key][zz] = np.inf
        for key in ("lower_contacts", "upper_contacts", "n_outside"):
            g[key][zz] = 0
    s_shared = s
    if sleep_mutation == "sleeper_fixed":                                # the sleeper as a fixed body in every shared denominator
        s_shared = dict(s, inverse_mass=keep(im, im * 0), inverse_inertia=keep(M, M * 0))
    n_sleeper_points = np.zeros(n, dtype=np.int64)

    # 4. pair contacts, Jacobi: every point from the poses after step 3, a body applies the average of its points
    inc, ref, pair, p_inc, p_ref = manifold_points(manifolds)
    branch, pair_cond = g["branch"].copy(), np.full(n, np.inf)
    sum_p, sum_q, count = pos * 0, rot * 0, np.zeros(n, dtype=np.int64)
    if inc:
        inc, ref, pair = np.array(inc), np.array(ref), np.array(pair)
        c0, surface = np.stack(p_inc, axis=1), np.stack(p_ref, axis=1)
        if c0.dtype == np.float64:
            c0, surface = num.conv(c0), num.conv(surface)
        correction = surface - c0
        cc = dot(correction, correction)
        delta = (frame_delta(p1_p[:, inc], p1_q[:, inc], past_p[:, inc], past_rot[:, inc], c0)
                 - frame_delta(p1_p[:, ref], p1_q[:, ref], past_p[:, ref], past_rot[:, ref], surface))
        tangential = delta - correction * (dot(delta, correction) / cc)                 # collision.rs:24-29, two bodies
        k, gap = np.ones(len(inc)), np.full(len(inc), np.inf)
        if mu is not None:
            point_mu = np.minimum(np.asarray(mu, dtype=np.float64)[inc], np.asarray(mu, dtype=np.float64)[ref])
            against = cc
            if mutation == "friction_against_distance":
                full = correction - tangential
                against = dot(full, full)
            k, gap = xm.friction_factor(num, point_mu, correction, tangential, against)
        if mutation == "tangential_dropped":
            k = k * 0
        c1 = surface - tangential * k
        diff = c1 - c0                                                                   # constraint.rs:13-23
        dist = sqrt(dot(diff, diff))
        direction = diff / dist
        Mi, Mr = M[:, :, inc], M[:, :, ref]
        if mutation == "transposed_inertia":
            Mi, Mr = Mi.transpose(1, 0, 2), Mr.transpose(1, 0, 2)
        origin_i, origin_r = pos[:, inc] + com[:, inc], pos[:, ref] + com[:, ref]       # rigid.rs:113-123, position + com
        if mutation == "arm_without_com":
            origin_i, origin_r = pos[:, inc], pos[:, ref]
        arm_i, arm_r = c0 - origin_i, surface - origin_r
        ai = qrot(conj(rot[:, inc]), cross(arm_i, direction))                           # constraint.rs:25-32
        ar = qrot(conj(rot[:, ref]), cross(arm_r, direction))
        im_w, M_w = s_shared["inverse_mass"], s_shared["inverse_inertia"]
        Mi_w, Mr_w = (Mi, Mr) if s_shared is s else (M_w[:, :, inc], M_w[:, :, ref])
        w = im_w[inc] + dot(matvec(Mi_w, ai), ai) + im_w[ref] + dot(matvec(Mr_w, ar), ar)
        error, clamp = xm.limited(num, dist, limit, delta, correction, cc)
        lam = error / (w + compliance)
        impulse_i = direction * lam                                                      # +lambda dir on the incident body at c0
        impulse_r = direction * (lam if mutation == "reference_sign" else -lam)          # -lambda dir on the reference body
        dpos_i, dpos_r = impulse_i * im[inc], impulse_r * im[ref]
        drot_i = qmul(pure(cross(matvec(Mi, arm_i), impulse_i)) * 0.5, rot[:, inc])     # rigid.rs:118-122
        drot_r = qmul(pure(cross(matvec(Mr, arm_r), impulse_r)) * 0.5, rot[:, ref])
        seen = set()
        d64 = num.to_f64(dist)
        both = np.minimum(gap, clamp)
        for t in range(len(inc)):
            for body, other, dp, dq in ((inc[t], ref[t], dpos_i[:, t], drot_i[:, t]), (ref[t], inc[t], dpos_r[:, t], drot_r[:, t])):
                sum_p[:, body] = sum_p[:, body] + dp
                sum_q[:, body] = sum_q[:, body] + dq
                if mutation != "average_by_pairs" or (body, pair[t]) not in seen:
                    count[body] += 1
                if zz[other]:
                    n_sleeper_points[body] += 1
                    count[body] += {"sleeper_point_twice": 1, "sleeper_point_uncounted": -1}.get(sleep_mutation, 0)
                seen.add((body, pair[t]))
                pair_cond[body] = min(pair_cond[body], d64[t])
                branch[body] = min(branch[body], both[t])
    if sleeping and sleep_mutation != "sleeper_share_applied":          # the sleeper's share: dropped, counted nowhere
        count[zz] = 0
    n_points = count.copy()
    # ... and the joints' entries, from the same poses, in the same average
    at = (integrated_pos, integrated_rot) if joint_mutation == "joints_from_integrated" else (pos, rot)
    joint_p, joint_q, joint_count, joint_info = joint_terms(
        num, s, at[0], at[1], joints, limits, compliance, limit, joint_mutation, drives=drives, past=(past_pos, past_rot),
        integrated=(integrated_pos, integrated_rot), h=hx)
    if len(joints):
        sum_p, sum_q, count = sum_p + joint_p, sum_q + joint_q, count + joint_count
        if sleeping and sleep_mutation != "sleeper_share_applied":
            count[zz] = 0
    hit = np.nonzero(count)[0]
    if len(hit):
        cnt = num.conv(count[hit].astype(np.float64))
        pos, rot = pos.copy(), rot.copy()
        pos[:, hit] = pos[:, hit] + sum_p[:, hit] / cnt
        rot[:, hit] = normalize_q(rot[:, hit] + sum_q[:, hit] / cnt, sqrt)

    # 5. Rigid::derive(past, h)                                             solver.rs:15
    vel, ang, _, flip_margin = xm.derive(num, pos, rot, past_pos, past_rot, hx)
    if sleeping and sleep_mutation != "sleeper_share_applied":          # no derive: what stage 6 reads of a sleeper is zero
        vel, ang = keep(vel, vel * 0), keep(ang, ang * 0)
        if sleep_mutation == "stage6_reads_stored_velocity":
            vel, ang = keep(vel, stored[2]), keep(ang, stored[3])

    # 6. restitution: a velocity pass on this substep's manifolds and ground mask          xpbd.h, "RESTITUTION"
    # 7. damping: joint dampers, drag, caps on what stage 6 left                            xpbd.h, "DAMPING"
    bounce_info = {}
    damp_mutation = mutation if mutation in DAMPING_MUTATIONS else None
    damped = damping is not None or (joint_damping is not None and len(joint_damping))

    def stage7(vel, ang):
        return damp(num, s, (pos, rot), (vel, ang), joints, damping, joint_damping, hx, damp_mutation,
                    (integrated_pos, integrated_rot))

    damp_info = {}
    if damped and damp_mutation == "stage7_before_stage6":
        vel, ang, damp_info = stage7(vel, ang)
    if restitution is not None or ground_restitution > 0:
        vel, ang, bounce_info = bounce(num, s_shared, (pos, rot), (vel, ang), (start_vel, start_ang), manifolds, g["mask"], vert, float(h),
                                       restitution, float(ground_restitution), bounce_threshold, terrain,
                                       mutation if mutation in BOUNCE_MUTATIONS else None, (integrated_pos, integrated_rot),
                                       g["xs"], compliance)
    if sleep_mutation == "sleeper_drag_applied":
        vel, ang = keep(vel, stored[2]), keep(ang, stored[3])
    if damped and damp_mutation != "stage7_before_stage6":
        vel, ang, damp_info = stage7(vel, ang)
    sleep_info = {}
    if sleeping:                                                          # rule (b): the input's bits
        if sleep_mutation != "sleeper_share_applied":
            pos, rot = keep(pos, stored[0]), keep(rot, stored[1])
            if sleep_mutation != "sleeper_drag_applied":
                vel, ang = keep(vel, stored[2]), keep(ang, stored[3])
        if contact_mask is not None:
            g["mask"][zz] = np.asarray(contact_mask, dtype=np.uint32)[zz]
        sleep_info = {"n_sleeper_points": n_sleeper_points, "asleep": zz}
        for key in ("bounce_pair_entries", "bounce_one_point", "bounce_ground_entries", "bounce_push", "bounce_give_back", "bounce_clamped"):
            if key in bounce_info:                                        # a sleeper's entry is dropped: it has none
                bounce_info[key][zz] = 0
    s.update(position=pos, rotation=rot, velocity=vel, angular_velocity=ang)
    return {"state": xm._pack(s), "frames": frames, "manifolds": manifolds, "undecided": undecided, "mask": g["mask"],
            "margin": g["margin"], "cond": g["cond"], "flip_margin": flip_margin, "domain": domain, "branch": branch,
            "pair_cond": pair_cond, "n_points": n_points, **joint_info, **bounce_info, **kin_info, **damp_info, **sleep_info,
            **{k: g[k] for k in ("cell_margin", "diagonal_margin", "border_margin", "lower_contacts", "upper_contacts", "n_outside")}}
