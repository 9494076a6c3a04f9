"""Independent f64 model of the sweep queries (include/xpbd.h, "Sweep queries"): every sweep against the bodies on the CPU.

A translating convex polytope against a resting one: over every axis of the SAT -- the faces of the volume, the faces of the body,
both signs of every pair of unique edge directions -- the separation is linear in t, s + t * v, and the time of impact is the
ray's slab test over those constraints, in the order of the definition.  Frames and planes are built as tests/raycast_model.py
builds them (Rigid::frame, Frame::inverse, Polytope::plane; cgmath's operation order, no fused multiply-add); the unique edge
directions come from the oracle's op_edge_directions.  Nothing here shares code with the library.

Polytopes are dicts as capi.World.set_polytopes takes them; bodies are (n, 38) xpbd_rigid rows; sweeps are records with the
fields position, rotation, direction, max_distance, shape, ignore_body, mask."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob
import raycast_model as rm
from overlap_model import oracle_polytope, shape_radius  # noqa: F401 (the oracle's Polytope of a dict; max |vertex - centroid|)

NO_HIT = 0xFFFFFFFF
FEATURE_FACE_A, FEATURE_FACE_B, FEATURE_EDGES, SWEEP_INITIAL = 0, 1, 2, 3
HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("face", "<u4"), ("reserved", "<u4"), ("distance", "<f8"),
                      ("position", "<f8", (3,)), ("normal", "<f8", (3,))])
INF = float("inf")


def edge_directions(poly):
    """(D, 3) unique edge directions of a polytope: the oracle's op_edge_directions."""
    L = ob.load()
    L.op_edge_directions.restype = C.c_uint32
    L.op_edge_directions.argtypes = [C.POINTER(ob.Polytope), C.POINTER(ob.Vec3), C.POINTER(C.c_uint32)]
    p = oracle_polytope(poly)
    dirs, of_edge = (ob.Vec3 * 64)(), (C.c_uint32 * 64)()
    n = L.op_edge_directions(C.byref(p), dirs, of_edge)
    return np.array([[dirs[k].x, dirs[k].y, dirs[k].z] for k in range(n)], dtype=np.float64).reshape(-1, 3)


def cols(a):
    """The three columns of an (N, 3) array as a tuple (what rm.rotate, rm.dot and rm.cross take)."""
    return (a[:, 0], a[:, 1], a[:, 2])


def frame_mul(pos, q, v):
    """Frame * Vector3: rotation * v + position."""
    r = rm.rotate(q, v)
    return (r[0] + pos[0], r[1] + pos[1], r[2] + pos[2])


def frame_inverse(pos, q):
    qi = (q[0], -q[1], -q[2], -q[3])
    return rm.rotate(qi, (-pos[0], -pos[1], -pos[2])), qi


def first_min(values):
    """Per column of (V, N): the first row's value, replaced by a later one that is smaller."""
    low = values[0].copy()
    for x in values[1:]:
        low = np.where(x < low, x, low)
    return low


def first_max(values):
    high = values[0].copy()
    for x in values[1:]:
        high = np.where(x > high, x, high)
    return high


class Shape:
    def __init__(self, poly):
        self.verts = np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3)
        self.planes = rm.polytope_planes(poly)
        self.dirs = edge_directions(poly)
        self.centroid = tuple(float(x) for x in poly["centroid"])
        self.radius = shape_radius(poly)


def slab(s, v, max_distance):
    """The ray's rule over the constraints (s[k], v[k]) in order: (hit, t, entering) -- entering None for an initial overlap."""
    if np.isnan(s).any() or np.isnan(v).any():
        return False, INF, None
    if ((v == 0.0) & (s >= 0.0)).any():
        return False, INF, None
    with np.errstate(all="ignore"):
        tk = (-s) / v
    t_lo, entering = -INF, None
    enter = np.where(v < 0.0, tk, -INF)
    enter = np.where(np.isnan(enter), -INF, enter)
    if enter.size:
        k = int(np.argmax(enter))                                          # the first maximum
        if enter[k] > t_lo:
            t_lo, entering = float(enter[k]), k
    t_hi = float(max_distance)
    for x in tk[v > 0.0]:
        if x < t_hi:
            t_hi = float(x)
    if t_lo < 0.0:
        t, entering = 0.0, None
    else:
        t = t_lo
    return t <= t_hi, t, entering


class Scene:
    """The bodies' side of the model, computed once and shared by the sweeps of a test."""

    def __init__(self, bodies, shape_id, polytopes, groups=None):
        self.shapes = [Shape(p) for p in polytopes]
        self.sid = [int(x) for x in shape_id]
        origin, rot = rm.body_frames(bodies)
        self.pos = [tuple(float(origin[a, i]) for a in range(3)) for i in range(len(self.sid))]
        self.rot = [tuple(float(rot[a, i]) for a in range(4)) for i in range(len(self.sid))]
        self.finite = np.isfinite(origin).all(axis=0) & np.isfinite(rot).all(axis=0)
        self.centres = np.array([frame_mul(self.pos[i], self.rot[i], self.shapes[s].centroid) for i, s in enumerate(self.sid)]).reshape(-1, 3)
        self.finite &= np.isfinite(self.centres).all(axis=1)
        self.body_radius = np.array([self.shapes[s].radius for s in self.sid])
        self.groups = None if groups is None else [int(g) for g in groups]
        self._world = {}

    def body_world(self, i):
        """World-space vertices of body i, (3 columns), and its inverse frame."""
        if i not in self._world:
            bw = frame_mul(self.pos[i], self.rot[i], cols(self.shapes[self.sid[i]].verts))
            self._world[i] = (bw, frame_inverse(self.pos[i], self.rot[i]))
        return self._world[i]

    def pair(self, vol, i, max_distance):
        """One (sweep, body) pair: (hit, t, what) -- what = (feature, face, normal), or None for a miss or an initial overlap."""
        A, B = vol["shape"], self.shapes[self.sid[i]]
        qa, qb = vol["rot"], self.rot[i]
        bw, (ipb, qib) = self.body_world(i)
        aw, d = vol["aw"], vol["d"]
        a_in_b = frame_mul(ipb, qib, aw)
        b_in_a = frame_mul(vol["ip"], vol["qi"], bw)
        d_b = rm.rotate(qib, d)
        s_parts, v_parts = [], []
        # 1. faces of the volume against the body's vertices in the volume's space
        n = cols(A.planes)
        low = first_min([rm.dot(n, (b_in_a[0][k], b_in_a[1][k], b_in_a[2][k])) for k in range(len(B.verts))])
        s_parts.append(low - A.planes[:, 3])
        v_parts.append(-rm.dot(n, vol["d_a"]))
        # 2. faces of the body against the volume's vertices in the body's space
        n = cols(B.planes)
        low = first_min([rm.dot(n, (a_in_b[0][k], a_in_b[1][k], a_in_b[2][k])) for k in range(len(A.verts))])
        s_parts.append(low - B.planes[:, 3])
        v_parts.append(rm.dot(n, d_b))
        # 3. pairs of unique edge directions, q = i * n_dirs_b + j, two constraints each
        ra = np.array(rm.rotate(qa, cols(A.dirs))).T.reshape(-1, 3)
        rb = np.array(rm.rotate(qb, cols(B.dirs))).T.reshape(-1, 3)
        ea, eb = np.repeat(ra, len(rb), axis=0), np.tile(rb, (len(ra), 1))
        with np.errstate(all="ignore"):
            c = rm.cross(cols(ea), cols(eb))
            inv_len = 1.0 / np.sqrt(rm.dot(c, c))
            n = (c[0] * inv_len, c[1] * inv_len, c[2] * inv_len)
            axis = np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2])
            da = [rm.dot((aw[0][k], aw[1][k], aw[2][k]), n) for k in range(len(A.verts))]
            db = [rm.dot((bw[0][k], bw[1][k], bw[2][k]), n) for k in range(len(B.verts))]
            hi_a, lo_a, hi_b, lo_b = first_max(da), first_min(da), first_max(db), first_min(db)
            w = rm.dot(n, d)
            se = np.stack([lo_b - hi_a, lo_a - hi_b], axis=1)[axis].reshape(-1)
            ve = np.stack([-w, w], axis=1)[axis].reshape(-1)
        edge_of = np.repeat(np.nonzero(axis)[0], 2)                          # the pair of every edge constraint kept
        s_parts.append(se)
        v_parts.append(ve)
        hit, t, entering = slab(np.concatenate(s_parts), np.concatenate(v_parts), max_distance)
        if not hit or entering is None:
            return hit, t, None
        fa, fb = len(A.planes), len(B.planes)
        if entering < fa:
            nk = tuple(float(x) for x in A.planes[entering, :3])
            r = rm.rotate(qa, nk)
            return True, t, (FEATURE_FACE_A, entering, (-r[0], -r[1], -r[2]))
        if entering < fa + fb:
            nk = tuple(float(x) for x in B.planes[entering - fa, :3])
            return True, t, (FEATURE_FACE_B, entering - fa, rm.rotate(qb, nk))
        e = entering - fa - fb
        q = int(edge_of[e])
        nq = (float(n[0][q]), float(n[1][q]), float(n[2][q]))
        return True, t, (FEATURE_EDGES, NO_HIT, nq if e & 1 else (-nq[0], -nq[1], -nq[2]))

    def volume(self, q):
        """The sweep's side of every pair, or None for a sweep that hits nothing."""
        sq = int(q["shape"])
        if sq >= len(self.shapes):
            return None
        pos = tuple(float(x) for x in q["position"])
        rot = tuple(float(x) for x in q["rotation"])
        d = tuple(float(x) for x in q["direction"])
        tmax = float(q["max_distance"])
        if not all(math.isfinite(x) for x in pos + rot + d) or d == (0.0, 0.0, 0.0) or not tmax >= 0.0:
            return None
        A = self.shapes[sq]
        centre = frame_mul(pos, rot, A.centroid)
        if not all(math.isfinite(x) for x in centre):
            return None
        ip, qi = frame_inverse(pos, rot)
        return {"shape": A, "pos": pos, "rot": rot, "d": d, "tmax": tmax, "aw": frame_mul(pos, rot, cols(A.verts)), "ip": ip, "qi": qi,
                "d_a": rm.rotate(qi, d), "centre": np.array(centre)}

    def sweep_one(self, q, masked=False):
        """(body, t, what) of one sweep record: what = (feature, face, normal) or None for an initial overlap; body None: a miss."""
        vol = self.volume(q)
        if vol is None:
            return None, INF, None
        # candidates, soonest first by a LOWER bound of the time their bounding spheres (0.1 % larger) meet: a body whose bound lies
        # beyond the best t cannot win.  This only saves work; every decision is pair()'s.
        d = np.array(vol["d"])
        with np.errstate(all="ignore"):
            w = self.centres - vol["centre"]
            reach = (vol["shape"].radius + self.body_radius) * 1.001 + 1e-9
            w2, wd, dd = (w * w).sum(axis=1), w @ d, float(d @ d)
            disc = wd * wd - dd * (w2 - reach * reach)
            t_in = np.where(w2 <= reach * reach, 0.0, (wd - np.sqrt(disc)) / dd)
            t_in = np.where((disc < 0.0) | (t_in < 0.0) & (w2 > reach * reach), INF, t_in)
            bound = t_in * (1.0 - 1e-9) - 1e-12
            bound = np.where(self.finite & np.isfinite(bound) & (bound <= vol["tmax"]), bound, INF)
        order = np.argsort(bound, kind="stable")
        ignore, mask = int(q["ignore_body"]), int(q["mask"])
        best = (None, INF, None)
        for i in order:
            i = int(i)
            if bound[i] == INF or bound[i] > best[1]:
                break
            if i == ignore:
                continue
            if masked and ((0xFFFFFFFF if self.groups is None else self.groups[i]) & mask) == 0:
                continue
            hit, t, what = self.pair(vol, i, vol["tmax"])
            if hit and (t < best[1] or (t == best[1] and (best[0] is None or i < best[0]))):
                best = (i, t, what)
        return best

    def sweep(self, sweeps, masked=False):
        """HIT_DTYPE records as the library returns them."""
        sweeps = np.asarray(sweeps).reshape(-1)
        out = np.zeros(len(sweeps), dtype=HIT_DTYPE)
        out["body"], out["face"], out["distance"] = NO_HIT, NO_HIT, INF
        for k, q in enumerate(sweeps):
            body, t, what = self.sweep_one(q, masked)
            if body is None:
                continue
            out["body"][k], out["distance"][k] = body, t
            out["position"][k] = [float(q["position"][a]) + float(q["direction"][a]) * t for a in range(3)]
            if what is None:
                out["feature"][k] = SWEEP_INITIAL
            else:
                out["feature"][k], out["face"][k], out["normal"][k] = what[0], what[1], what[2]
        return out


def sweep(bodies, shape_id, polytopes, sweeps, masked=False, groups=None):
    return Scene(bodies, shape_id, polytopes, groups).sweep(sweeps, masked)
