"""Extended-precision model of solver::step for independent bodies on the ground plane.

A second reading of the reference's semantics, written from the reference and nothing else: it does not call or read
oracle/ or the host mirror, and it does not follow their f64 operation order.  Bit-identity with oracle/xpbd_oracle.c
pins the kernels' operation order; this model pins what the operations MEAN: an implementation that only reorders f64
arithmetic stays within a rounding bound of it (tests/xprec_cases.py), one that misreads the reference (a transposed
matrix, a dropped term, a wrong compliance) does not.

Written once, generic over the scalar: every quantity is a numpy array over bodies, either of np.longdouble (64-bit
significand on x86-64, 2^11 times finer than f64: the fast path) or of mpmath.mpf objects (the check path).  Vectors are
arrays (3, n), quaternions (4, n) as (s, x, y, z), matrices (3, 3, n) indexed [column, row] (cgmath Matrix3, the ABI's
[3*col + row]).

Reference lines below are jim-ec/constraint_solver src/*.rs.  The terrain (terrain_lookup, ground(terrain=)) is the one
extension here: a second reading of include/xpbd.h, "TERRAIN", alone, generic over the scalar like the rest.
"""
import numpy as np

# f64 limits the model uses to decide where the f64 reference leaves its domain (NaN/Inf or a lost square)
F64_MIN_NORMAL = 2.0 ** -1022


class Num:
    """The scalar type: `conv` turns an f64 array into model scalars exactly, `sqrt` is the type's square root, `atan2` its
    two-argument arc tangent (the angular joint limits), `tan` its tangent (the kinematic overwrite)."""

    def __init__(self, name, conv, sqrt, to_f64, const, atan2=np.arctan2, tan=np.tan):
        self.name, self.conv, self.sqrt, self.to_f64, self.const, self.atan2, self.tan = name, conv, sqrt, to_f64, const, atan2, tan


def longdouble():
    return Num("longdouble", lambda a: np.asarray(a, dtype=np.float64).astype(np.longdouble), np.sqrt,
               lambda a: np.asarray(a, dtype=np.longdouble).astype(np.float64), np.longdouble)


def f64():
    """Plain f64 (np.float64, np.sqrt, np.arctan2): the model's text evaluated as one more f64 implementation, with the
    model's operation order and numpy's libm.  Not a reference: a comparand."""
    return Num("f64", lambda a: np.array(a, dtype=np.float64), np.sqrt, lambda a: np.asarray(a, dtype=np.float64), np.float64)


def mp(digits=40):
    import mpmath
    ctx = mpmath.mp.clone() if hasattr(mpmath.mp, "clone") else mpmath.mp
    ctx.dps = digits
    mpf = ctx.mpf
    conv = np.frompyfunc(lambda x: mpf(float(x)), 1, 1)
    back = np.frompyfunc(float, 1, 1)
    return Num("mpmath%d" % digits, lambda a: conv(np.asarray(a, dtype=np.float64)).astype(object),
               np.frompyfunc(ctx.sqrt, 1, 1), lambda a: back(np.asarray(a, dtype=object)).astype(np.float64), mpf,
               np.frompyfunc(ctx.atan2, 2, 1), np.frompyfunc(ctx.tan, 1, 1))


def native():
    """The model's own hardware precision: longdouble if it is finer than f64 by 2^10 or more, else mpmath."""
    return longdouble() if np.finfo(np.longdouble).nmant >= 63 else mp(40)


def lifted(ref, a):
    """A longdouble array in another scalar type, exactly: two doubles."""
    hi = np.asarray(a).astype(np.float64)
    lo = (a - hi.astype(a.dtype)).astype(np.float64)
    return ref.conv(hi) + ref.conv(lo)


# ---- cgmath semantics (cgmath 0.18: Vector3, Quaternion, Matrix3) ---------------------------------------------------
def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def qmul(a, b):
    return np.stack([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def qrot(q, v):
    """Quaternion * Vector3 (cgmath): v + 2 u x (u x v + s v), u = q.v -- the rotation of v for a unit q."""
    u = q[1:]
    return cross(u, cross(u, v) + v * q[0]) * 2 + v


def conj(q):
    return np.concatenate([q[:1], -q[1:]])


def pure(v):
    """Quaternion::from_sv(0, v)."""
    return np.concatenate([v[:1] * 0, v])


def matvec(m, v):
    """Matrix3 * Vector3 with m[column, row]: sum over columns of column * component."""
    return m[0] * v[0] + m[1] * v[1] + m[2] * v[2]


def normalize_q(q, sqrt):
    return q / sqrt(dot(q[1:], q[1:]) + q[0] * q[0])


# ---- Frame (frame.rs) -------------------------------------------------------------------------------------------------
def frame_apply(fp, fq, v):
    """Frame * Vector3 = rotation * v + position (frame.rs:47-53)."""
    return qrot(fq, v) + fp


def frame_delta(cp, cq, pp, pq, g):
    """Frame::delta (frame.rs:40-44): global - past * (self.inverse() * global); inverse is frame.rs:30-37."""
    iq = conj(cq)
    local = qrot(iq, g) + qrot(iq, -cp)
    return g - frame_apply(pp, pq, local)


# ---- the step ---------------------------------------------------------------------------------------------------------
FIELDS = {"inverse_mass": (0, 1), "inverse_inertia": (1, 10), "external_force": (10, 13), "internal_force": (13, 16),
          "external_torque": (16, 19), "internal_torque": (19, 22), "velocity": (22, 25), "angular_velocity": (25, 28),
          "center_of_mass": (28, 31), "position": (31, 34), "rotation": (34, 38)}


def _unpack(bodies, num):
    b = (bodies if carried(bodies) else num.conv(np.ascontiguousarray(bodies, dtype=np.float64))).reshape(-1, 38).T
    s = {k: b[lo:hi] for k, (lo, hi) in FIELDS.items()}
    s["inverse_mass"] = b[0]
    s["inverse_inertia"] = b[1:10].reshape(3, 3, -1)                                      # [col, row, body]
    return s


def carried(bodies):
    """A state already in model scalars (the `state` of an earlier step), carried on without rounding to f64."""
    return isinstance(bodies, np.ndarray) and bodies.dtype in (np.dtype(np.longdouble), np.dtype(object))


def _pack(s):
    n = s["position"].shape[1]
    rows = [s["inverse_mass"][None]] + [s[k].reshape(-1, n) for k in list(FIELDS)[1:]]
    return np.concatenate(rows).T                                                         # (n, 38) model scalars


def shape_table(verts, offsets, shape_id):
    """Per-body vertex slots: (n, 32, 3) f64, zero-padded, and the vertex count of every body."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    sid = np.asarray(shape_id, dtype=np.int64)
    counts = (offsets[1:] - offsets[:-1])[sid]
    slots = np.zeros((len(sid), 32, 3))
    for k in range(len(offsets) - 1):
        sel = sid == k
        nv = offsets[k + 1] - offsets[k]
        slots[sel, :nv] = verts[offsets[k]:offsets[k + 1]]
    return slots, counts


def integrate(s, pos, rot, vel, ang, h, sqrt):
    """Rigid::integrate, rigid.rs:82-99, for every body of the unpacked state `s`."""
    im, M = s["inverse_mass"], s["inverse_inertia"]
    force = s["external_force"] + qrot(rot, s["internal_force"])
    vel = vel + force * h * im
    pos = pos + vel * h
    torque = s["external_torque"] + qrot(rot, s["internal_torque"])
    ang = ang + matvec(M, torque) * h
    rot = normalize_q(rot + qmul(pure(ang) * (h / 2), rot), sqrt)
    return pos, rot, vel, ang


def friction_factor(num, mu, correction, tangential, cc):
    """include/xpbd.h, "Contact MATERIALS": the contact takes back at most mu |correction| of the tangential slip.  Returns
    (k, |bound - slip| in metres; inf where mu is +inf).  mu: f64 array over the contacts."""
    sqrt = num.sqrt
    finite = np.isfinite(mu)
    len_c, len_t = sqrt(cc), sqrt(dot(tangential, tangential))
    bound = num.conv(np.where(finite, mu, 0.0)) * len_c
    slides = finite & (bound < len_t).astype(bool)
    k = np.where(slides, bound / np.where(slides, len_t, len_t * 0 + 1), len_t * 0 + 1)
    return k, np.where(finite, np.abs(num.to_f64(bound - len_t)), np.inf)


def limited(num, dist, limit, delta, correction, cc):
    """oracle/xpbd_pairs_oracle.h, op_contacts_set_max_depenetration_speed: the constraint's length is limited to
    max(0, speed h - closing), closing = delta . correction / |correction|.  limit = speed h, None = off.  Returns (the
    length to remove, |dist - allowed| in metres; inf when off)."""
    if limit is None:
        return dist, np.full(dist.shape, np.inf)
    allowed = limit - dot(delta, correction) / num.sqrt(cc)
    allowed = np.where((allowed > 0).astype(bool), allowed, allowed * 0)
    return np.where((dist > allowed).astype(bool), allowed, dist), np.abs(num.to_f64(dist - allowed))


TERRAIN_MUTATIONS = ("triangles_swapped", "target_vertical", "d_unnormalised", "plane_beyond_field")


def heightfield(heights, origin, cell):
    """The terrain of include/xpbd.h, "TERRAIN", as the model takes it: heights (ny, nx) f64, H[j][i] = heights[j, i]."""
    return {"heights": np.ascontiguousarray(heights, dtype=np.float64), "origin": (float(origin[0]), float(origin[1])),
            "cell": (float(cell[0]), float(cell[1]))}


def _floor(num, u):
    """floor(u) as an f64 array (whole numbers are exact in every scalar type), decided in the model's scalars."""
    f = np.floor(num.to_f64(u))
    f = np.where((num.conv(f) > u).astype(bool), f - 1, f)
    return np.where((num.conv(f + 1) <= u).astype(bool), f + 1, f)


def terrain_lookup(num, terrain, x, mutation=None):
    """include/xpbd.h, "TERRAIN", "Lookup", steps 1 to 6, for the world points x (3, k); written from that prose alone, not
    from tests/terrain_model.py or the kernels.  Returns (inside (k,) bool -- False is the header's OUTSIDE --, n (3, k),
    d (k,), info): the plane {n, d} of the triangle above or below each point (a stand-in where it is outside), and in
    `info` per point `lower` (bool, the triangle of step 4) and, in metres and f64, the distances at which the plane changes
    discretely: `cell` from the nearest cell line, `diagonal` from the line fu == fv of its cell, `border` from the field's
    border (for points outside too)."""
    assert mutation is None or mutation in TERRAIN_MUTATIONS
    H = terrain["heights"]
    ny, nx = H.shape
    x0, y0 = (num.conv(np.array([c]))[0] for c in terrain["origin"])
    dx, dy = (num.conv(np.array([c]))[0] for c in terrain["cell"])
    u, v = (x[0] - x0) / dx, (x[1] - y0) / dy                                          # 1.
    inside = (u >= 0).astype(bool) & (v >= 0).astype(bool)
    safe_u, safe_v = np.where(inside, u, u * 0), np.where(inside, v, v * 0)
    fi, fj = _floor(num, safe_u), _floor(num, safe_v)                                  # 2. half-open at the far edges
    inside = inside & (fi < nx - 1) & (fj < ny - 1)
    fi, fj = np.where(inside, fi, 0.0), np.where(inside, fj, 0.0)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    fu, fv = safe_u - num.conv(fi), safe_v - num.conv(fj)                              # 3.
    h00, h10, h01, h11 = (num.conv(H[j + a, i + b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)))
    lower = (fu >= fv).astype(bool)                                                    # 4. the diagonal belongs to the lower one
    if mutation == "triangles_swapped":
        lower = ~lower
    sx = np.where(lower, (h10 - h00) / dx, (h11 - h01) / dx)
    sy = np.where(lower, (h11 - h10) / dy, (h01 - h00) / dy)
    raw = np.stack([-sx, -sy, sx * 0 + 1])                                             # 5.
    n = raw * ((sx * 0 + 1) / num.sqrt(dot(raw, raw)))                                 # raw * (1.0 / length(raw))
    corner = np.stack([x0 + num.conv(fi) * dx, y0 + num.conv(fj) * dy, h00])           # 6.
    d = dot(raw if mutation == "d_unnormalised" else n, corner)
    # how far the point is from where the plane changes (f64, metres)
    u64, v64, fu64, fv64 = (np.asarray(num.to_f64(a), dtype=np.float64) for a in (u, v, fu, fv))
    cx, cy = terrain["cell"]
    cell = np.minimum(np.minimum(fu64, 1 - fu64) * cx, np.minimum(fv64, 1 - fv64) * cy)
    diagonal = np.abs(fu64 - fv64) * cx * cy / np.hypot(cx, cy)
    px, py, lx, ly = u64 * cx, v64 * cy, (nx - 1) * cx, (ny - 1) * cy
    within = (px >= 0) & (py >= 0) & (px <= lx) & (py <= ly)
    out_x, out_y = np.maximum(np.maximum(-px, px - lx), 0), np.maximum(np.maximum(-py, py - ly), 0)
    border = np.where(within, np.minimum(np.minimum(px, lx - px), np.minimum(py, ly - py)), np.hypot(out_x, out_y))
    border = np.where(np.isnan(border), 0.0, border)
    info = {"lower": lower, "cell": np.where(inside, cell, np.inf), "diagonal": np.where(inside, diagonal, np.inf), "border": border}
    if mutation == "plane_beyond_field":                                               # the plane z = 0 wherever the field is not
        n = np.where(inside, n, np.stack([sx * 0, sx * 0, sx * 0 + 1]))
        d = np.where(inside, d, d * 0)
        inside = np.ones_like(inside)
    return inside, n, d, info


def ground(num, s, pos, rot, past_p, past_rot, vert, counts, compliance, domain, mu=None, limit=None, terrain=None, mutation=None):
    """collision::ground and solver::solve for every body, from the post-integrate pose (pos, rot).  mu (f64 per body) and
    limit (speed h) are the extension's friction and depenetration limit; None is the reference.  terrain (heightfield()):
    the plane under each vertex is the lookup's {n, d} in place of z = 0 (xpbd.h, "TERRAIN", "Ground contacts"): the vertex
    contacts iff it is inside the field and !(s >= 0), s = dot(n, x) - d; target = x - s n; everything after `target` is the
    code of the plane.  mutation: one of TERRAIN_MUTATIONS.  Returns the pose after the solve and the masks, margins and
    conditioning of step(); `margin` is min |s| with a terrain (inside vertices), and cell_margin, diagonal_margin and
    border_margin the smallest terrain_lookup distances of a tested vertex; lower_contacts / upper_contacts count the body's
    contacts by triangle and n_outside its vertices outside the field."""
    sqrt = num.sqrt
    im, M, com = s["inverse_mass"], s["inverse_inertia"], s["center_of_mass"]
    n, vmax = pos.shape[1], len(vert)
    # collision::ground, collision.rs:13-35: every constraint is built from this post-integrate frame
    cur_p, cur_q = pos + com + qrot(rot, -com), rot
    mask = np.zeros(n, dtype=np.uint32)
    margin = np.full(n, np.inf)
    branch = np.full(n, np.inf)
    lines = {k: np.full(n, np.inf) for k in ("cell_margin", "diagonal_margin", "border_margin")}
    tally = {k: np.zeros(n, dtype=np.int64) for k in ("lower_contacts", "upper_contacts", "n_outside")}
    xs, planes = [], []
    for v in range(vmax):
        x = frame_apply(cur_p, cur_q, vert[v])                              # collision.rs:17
        live = v < counts
        if terrain is None:
            z = num.to_f64(x[2])
            below = live & (x[2] < 0).astype(bool)                          # collision.rs:18, skip when z >= 0
            planes.append(None)
        else:
            inside, pn, pd, where = terrain_lookup(num, terrain, x, mutation if mutation in TERRAIN_MUTATIONS else None)
            dist = dot(pn, x) - pd
            z = np.where(inside, num.to_f64(dist), np.inf)
            below = live & inside & ~(dist >= 0).astype(bool)
            planes.append((pn, dist))
            for key, name in (("cell_margin", "cell"), ("diagonal_margin", "diagonal"), ("border_margin", "border")):
                lines[key] = np.where(live, np.minimum(lines[key], where[name]), lines[key])
            tally["lower_contacts"] += below & where["lower"]
            tally["upper_contacts"] += below & ~where["lower"]
            tally["n_outside"] += live & ~inside
        margin = np.where(live, np.minimum(margin, np.abs(z)), margin)
        mask |= below.astype(np.uint32) << np.uint32(v)
        xs.append(x)

    # solver::solve, solver.rs:19-27: the constraints in push order, each against the live pose
    cond = np.full(n, np.inf)
    pos, rot = pos.copy(), rot.copy()               # the live pose; cur_p and cur_q stay frozen
    for v in range(vmax):
        idx = np.nonzero((mask >> np.uint32(v)) & 1)[0]
        if not len(idx):
            continue
        x = xs[v][:, idx]
        p_, q_, M_, c_, im_ = pos[:, idx], rot[:, idx], M[:, :, idx], com[:, idx], im[idx]
        if terrain is None:
            target = np.stack([x[0], x[1], x[2] * 0])                      # collision.rs:22
        else:
            pn, dist = planes[v][0][:, idx], planes[v][1][idx]
            target = x - pn * dist                                          # xpbd.h: target = x - s * n per component
            if mutation == "target_vertical":                               # the surface point straight below or above x
                target = np.stack([x[0], x[1], x[2] - dist / pn[2]])
        correction = target - x                                             # collision.rs:23
        cc = dot(correction, correction)
        domain[idx] &= num.to_f64(cc) >= F64_MIN_NORMAL
        cc = np.where(num.to_f64(cc) > 0, cc, cc + 1)                       # only out-of-domain bodies reach 0
        delta = frame_delta(cur_p[:, idx], cur_q[:, idx], past_p[:, idx], past_rot[:, idx], x)   # collision.rs:24
        tangential = delta - correction * (dot(delta, correction) / cc)    # collision.rs:25, project_on
        if mu is not None:
            k, gap = friction_factor(num, mu[idx], correction, tangential, cc)
            branch[idx] = np.minimum(branch[idx], gap)
            tangential = tangential * k
        c0, c1 = x, target - tangential                                     # collision.rs:27-31, distance 0
        diff = c1 - c0                                                      # constraint.rs:13-15
        dist = sqrt(dot(diff, diff))                                        # constraint.rs:21-23
        cond[idx] = np.minimum(cond[idx], num.to_f64(dist))
        dist = np.where(num.to_f64(dist) > 0, dist, dist + 1)
        direction = diff / dist                                             # constraint.rs:17-19
        # inverse_resitance, constraint.rs:25-32: the arm is taken into rest space
        ai = qrot(conj(q_), cross(c0 - (p_ + c_), direction))
        w = im_ + dot(matvec(M_, ai), ai)
        error, gap = limited(num, dist, limit, delta, correction, cc)
        branch[idx] = np.minimum(branch[idx], gap)
        lam = error / (w + compliance)                                      # solver.rs:23-24 (distance == 0)
        impulse = direction * lam                                           # constraint.rs:34-37
        # Rigid::apply_impulse, rigid.rs:113-123: the world-space arm is NOT rotated into rest space
        p_ = p_ + impulse * im_
        spin = cross(matvec(M_, c0 - (p_ + c_)), impulse)
        q_ = normalize_q(q_ + qmul(pure(spin) * 0.5, q_), sqrt)
        pos[:, idx], rot[:, idx] = p_, q_
    return pos, rot, {"mask": mask, "margin": margin, "cond": cond, "branch": branch, "xs": xs, **lines, **tally}


def derive(num, pos, rot, past_pos, past_rot, h):
    """Rigid::derive, rigid.rs:101-109.  Returns velocity, angular velocity, the flip taken and |delta.s|."""
    vel = (pos - past_pos) / h
    dq = qmul(rot, conj(past_rot))
    flip = (dq[0] < 0).astype(bool)
    dq = np.where(flip, -dq, dq)
    return vel, dq[1:] * 2 / h, flip, np.abs(num.to_f64(dq[0]))


def step(bodies, verts, offsets, shape_id, dt, substeps, num=None):
    """solver::step (solver.rs:3-17) for every body, in the model's precision.  `bodies`: (n, 38) f64, converted
    exactly, or the `state` of an earlier call, carried on in the model's scalars.

    Returns a dict: `state` (n, 38) model scalars after the step; per substep (rows) and body (columns): `masks` (uint32,
    bit v = shape vertex v produced a ground constraint), `margin` (min |z| of the body's vertices at the ground test,
    f64), `cond` (smallest |c1 - c0| of a solved constraint, the conditioning of normalize; inf without one), `flip`
    (derive took its delta.s < 0 branch) and `flip_margin` (|delta.s|); and `domain` (n,) bool: False where the f64
    reference itself leaves its domain (non-finite or degenerate input, a constraint whose correction.correction is not a
    normal f64), so that the model does not describe it."""
    num = num or native()
    sqrt = num.sqrt
    b64 = np.asarray(num.to_f64(bodies) if carried(bodies) else bodies, dtype=np.float64).reshape(-1, 38)
    n = b64.shape[0]
    domain = np.isfinite(b64).all(axis=1) & (np.abs(b64[:, 34:38]).max(axis=1) > 0)
    if carried(bodies) and domain.all():
        s = _unpack(bodies, num)
    else:
        safe = b64.copy()
        safe[~domain] = 0.0                             # a benign stand-in keeps the vectorised arithmetic finite
        safe[~domain, 34] = 1.0
        s = _unpack(safe, num)
    slots, counts = shape_table(verts, offsets, shape_id)
    vmax = int(counts.max()) if n else 0
    vert = [num.conv(slots[:, v].T) for v in range(vmax)]

    com = s["center_of_mass"]
    pos, rot, vel, ang = s["position"], s["rotation"], s["velocity"], s["angular_velocity"]
    h = num.const(float(dt)) / substeps                  # solver.rs:4, dt / substep_count taken exactly
    compliance = num.const("1e-6") / (h * h)             # solver.rs:20

    out = {k: [] for k in ("masks", "margin", "cond", "flip", "flip_margin")}
    for _ in range(substeps):
        past_pos, past_rot = pos, rot                                           # solver.rs:7-8
        past_p = pos + com + qrot(rot, -com)                                    # solver.rs:9, Rigid::frame rigid.rs:75-80
        pos, rot, vel, ang = integrate(s, pos, rot, vel, ang, h, sqrt)
        pos, rot, g = ground(num, s, pos, rot, past_p, past_rot, vert, counts, compliance, domain)
        vel, ang, flip, flip_margin = derive(num, pos, rot, past_pos, past_rot, h)
        out["masks"].append(g["mask"])
        out["margin"].append(g["margin"])
        out["cond"].append(g["cond"])
        out["flip"].append(flip)
        out["flip_margin"].append(flip_margin)

    s.update(position=pos, rotation=rot, velocity=vel, angular_velocity=ang)
    res = {k: np.array(v) for k, v in out.items()}
    res["state"] = _pack(s)
    res["domain"] = domain
    return res


def extent(verts, offsets, shape_id, bodies):
    """Largest distance of a body's vertices from its position, |center_of_mass| included: the pose scale beyond |x|."""
    slots, counts = shape_table(verts, offsets, shape_id)
    r = np.linalg.norm(slots, axis=2).max(axis=1)
    return r + 2 * np.linalg.norm(np.asarray(bodies)[:, 28:31], axis=1)
