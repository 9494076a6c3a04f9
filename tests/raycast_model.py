"""Independent f64 model of the batched ray casts (include/xpbd.h, "Scene queries"), brute force in numpy.

Derived from the reference, not from the library's tables: a body's frame is Rigid::frame (src/rigid.rs:75-80), its
inverse Frame::inverse (src/frame.rs:30-37), a face plane Polytope::plane over Plane::from_points / facing / flip
(src/geometry.rs:16-24, 55-68, 262-271), recomputed here from the polytope's vertices.  Every expression keeps cgmath's
operation order (Quaternion * Vector3: t = v x w + w * s; v x t * 2 + w), and numpy never fuses a multiply-add, so the
results are those of an f64 evaluation of the semantics in that order.

Polytopes are dicts as capi.World.set_polytopes takes them: vertices (V, 3), face_offsets (F + 1), face_indices, centroid.
Bodies are (n, 38) xpbd_rigid rows.  Rays: origin (R, 3), direction (R, 3), max_distance (R,), ignore_body (R,)."""
import numpy as np

NO_HIT = 0xFFFFFFFF
RAY_INSIDE = 0xFFFFFFFF


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def rotate(q, v):
    """cgmath Quaternion * Vector3 with q = (s, x, y, z) and v = (x, y, z), components as arrays (broadcast)."""
    qv = (q[1], q[2], q[3])
    c = cross(qv, v)
    t = (c[0] + v[0] * q[0], c[1] + v[1] * q[0], c[2] + v[2] * q[0])
    c2 = cross(qv, t)
    return (c2[0] * 2.0 + v[0], c2[1] * 2.0 + v[1], c2[2] * 2.0 + v[2])


def polytope_planes(poly):
    """(F, 4) outward planes (normal, displacement) of a polytope: Polytope::plane for every face."""
    v = np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3)
    fo, fi = np.asarray(poly["face_offsets"]), np.asarray(poly["face_indices"])
    c = [float(x) for x in poly["centroid"]]
    out = np.zeros((len(fo) - 1, 4))
    for f in range(len(fo) - 1):
        p0, p1, p2 = (v[int(fi[fo[f] + k])] for k in range(3))
        e1, e2 = tuple(p1 - p0), tuple(p2 - p0)
        n = cross(e1, e2)
        inv_len = 1.0 / np.sqrt(dot(n, n))                                  # normalize: v * (1 / |v|)
        n = (n[0] * inv_len, n[1] * inv_len, n[2] * inv_len)
        disp = dot(n, tuple(p0))
        support = (disp * n[0], disp * n[1], disp * n[2])
        facing = dot(n, (c[0] - support[0], c[1] - support[1], c[2] - support[2])) >= 0.0
        if facing:                                                        # flip: the plane points away from the centroid
            n, disp = (-n[0], -n[1], -n[2]), -disp
        out[f] = (n[0], n[1], n[2], disp)
    return out


def body_frames(bodies):
    """Rigid::frame of every body: (origin (3, n), rotation (4, n))."""
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    pos, com, rot = b[:, 31:34].T, b[:, 28:31].T, b[:, 34:38].T
    neg = (-com[0], -com[1], -com[2])
    r = rotate(tuple(rot), neg)
    origin = np.array([(pos[a] + com[a]) + r[a] for a in range(3)])
    return origin, rot.copy()


def ray_valid(rays):
    o, d, m = rays["origin"], rays["direction"], rays["max_distance"]
    finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    return finite & (d != 0.0).any(axis=1) & (m >= 0.0)


def candidates(bodies, shape_id, polytopes, rays):
    """t (R, n) of every (ray, body) pair (+inf: no hit), the entering face (R, n) and whether the pair hits (R, n)."""
    rays = np.asarray(rays)
    R, n = len(rays), len(bodies)
    t_all = np.full((R, n), np.inf)
    face_all = np.full((R, n), NO_HIT, dtype=np.uint32)
    hit_all = np.zeros((R, n), dtype=bool)
    origin, rot = body_frames(bodies)
    finite = np.isfinite(origin).all(axis=0) & np.isfinite(rot).all(axis=0)
    qi = (rot[0], -rot[1], -rot[2], -rot[3])                              # conjugate
    ip = rotate(qi, (-origin[0], -origin[1], -origin[2]))                 # inverse position: qi * -position
    valid = ray_valid(rays)
    o = [rays["origin"][:, a][:, None] for a in range(3)]
    d = [rays["direction"][:, a][:, None] for a in range(3)]
    planes = [polytope_planes(p) for p in polytopes]
    sid = np.asarray(shape_id, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s, pl in enumerate(planes):
            cols = np.nonzero(sid == s)[0]
            if cols.size == 0:
                continue
            q = tuple(x[cols][None, :] for x in qi)
            r_o = rotate(q, tuple(o))
            o_l = tuple(r_o[a] + ip[a][cols][None, :] for a in range(3))
            d_l = rotate(q, tuple(d))
            shape = (R, cols.size)
            t_lo, t_hi = np.zeros(shape), np.broadcast_to(rays["max_distance"][:, None], shape).copy()
            face = np.full(shape, RAY_INSIDE, dtype=np.uint32)
            alive = np.ones(shape, dtype=bool)
            for k in range(len(pl)):
                nk = tuple(pl[k, :3])
                sk = dot(nk, o_l) - pl[k, 3]
                vk = dot(nk, d_l)
                alive &= ~(np.isnan(sk) | np.isnan(vk))
                tk = (-sk) / vk
                enter = (vk < 0.0) & (tk > t_lo)
                t_lo = np.where(enter, tk, t_lo)
                face = np.where(enter, np.uint32(k), face)
                leave = (vk > 0.0) & (tk < t_hi)
                t_hi = np.where(leave, tk, t_hi)
                alive &= ~((vk == 0.0) & (sk > 0.0))
            hit = alive & (t_lo <= t_hi) & valid[:, None] & finite[cols][None, :]
            t_all[:, cols] = np.where(hit, t_lo, np.inf)
            face_all[:, cols] = np.where(hit, face, np.uint32(NO_HIT))
            hit_all[:, cols] = hit
    ignore = rays["ignore_body"].astype(np.int64)
    rows = np.nonzero(ignore < n)[0]
    t_all[rows, ignore[rows]] = np.inf
    face_all[rows, ignore[rows]] = NO_HIT
    hit_all[rows, ignore[rows]] = False
    return t_all, face_all, hit_all


def raycast(bodies, shape_id, polytopes, rays):
    """Hits as a dict of arrays (body, face, distance, point (R, 3), normal (R, 3)) and the second-best t of every ray."""
    rays = np.asarray(rays)
    t_all, face_all, hit_any = candidates(bodies, shape_id, polytopes, rays)
    R, n = t_all.shape
    body = np.full(R, NO_HIT, dtype=np.uint32)
    second = np.full(R, np.inf)
    if n:
        best = np.argmin(t_all, axis=1)                                    # first index of the minimum: the smaller body wins
        rows = np.arange(R)
        got = hit_any[rows, best]
        body = np.where(got, best, NO_HIT).astype(np.uint32)
        masked = t_all.copy()
        masked[rows, best] = np.inf
        second = masked.min(axis=1)
    out = {"body": body, "face": np.full(R, NO_HIT, dtype=np.uint32), "distance": np.full(R, np.inf),
           "point": np.zeros((R, 3)), "normal": np.zeros((R, 3))}
    origin, rot = body_frames(bodies)
    planes = [polytope_planes(p) for p in polytopes]
    for r in np.nonzero(body != NO_HIT)[0]:
        i = int(body[r])
        t = t_all[r, i]
        f = int(face_all[r, i])
        out["face"][r], out["distance"][r] = f, t
        out["point"][r] = [rays["origin"][r, a] + rays["direction"][r, a] * t for a in range(3)]
        if f != RAY_INSIDE:
            nrm = planes[int(shape_id[i])][f, :3]
            out["normal"][r] = rotate(tuple(rot[:, i]), tuple(nrm))
    return out, second


# ---- shapes for the analytic checks ------------------------------------------------------------------------------------
def box(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]])
    faces = [[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [2, 3, 7, 6], [0, 4, 7, 3], [1, 2, 6, 5]]   # -z +z -y +y -x +x
    return _poly(v, faces)


def tetrahedron(scale=1.0):
    v = scale * np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return _poly(v, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def icosahedron(scale=1.0):
    from scipy.spatial import ConvexHull
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = []
    for a in (-1.0, 1.0):
        for b in (-g, g):
            v += [[0.0, a, b], [a, b, 0.0], [b, 0.0, a]]
    v = scale * np.array(v) / np.linalg.norm([1.0, g])
    return _poly(v, ConvexHull(v).simplices.tolist())


def _poly(v, faces):
    fo = np.cumsum([0] + [len(f) for f in faces]).astype(np.uint32)
    fi = np.array([i for f in faces for i in f], dtype=np.uint32)
    edges = sorted({tuple(sorted((f[k], f[(k + 1) % len(f)]))) for f in faces for k in range(len(f))})
    return {"vertices": np.asarray(v, dtype=np.float64), "edges": np.array(edges, dtype=np.uint32), "face_offsets": fo,
            "face_indices": fi, "centroid": np.asarray(v, dtype=np.float64).mean(axis=0)}


def rigid(position, rotation=(1.0, 0.0, 0.0, 0.0), com=(0.0, 0.0, 0.0)):
    """An xpbd_rigid row with the given pose and centre of mass (masses do not matter to a ray)."""
    b = np.zeros(38)
    b[0] = 1.0
    b[1], b[5], b[9] = 1.0, 1.0, 1.0
    b[28:31], b[31:34], b[34:38] = com, position, rotation
    return b
