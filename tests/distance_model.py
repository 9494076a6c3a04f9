"""Independent f64 model of the distance queries (include/xpbd.h, "Distance queries"): every query against the bodies on the CPU.

Written from the header's text.  One (volume, body) pair is the overlap query's decision first -- the tight spheres in plain
Python floats and the oracle's op_sat, as tests/overlap_model.py has them; for the point volume the deepest face plane -- and then
the first minimum of d2 over the candidate list of the definition: every vertex of the volume over every face of the body, every
vertex of the body over every face of the volume, every pair of edges as two clamped segments.  Frames and planes are built as
tests/raycast_model.py builds them (Rigid::frame, Frame::inverse, Polytope::plane; cgmath's operation order, and numpy never
fuses a multiply-add).  Nothing here shares code with the library.

Polytopes are dicts as capi.World.set_polytopes takes them; bodies are (n, 38) xpbd_rigid rows; queries are records with the
fields position, rotation, max_distance, shape, ignore_body, mask."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob
import overlap_model as om
import raycast_model as rm
from sweep_model import cols, first_max, frame_inverse, frame_mul

NO_HIT = 0xFFFFFFFF
POINT = 0xFFFFFFFF
FEATURE_FACE_A, FEATURE_FACE_B, FEATURE_EDGES, OVERLAP = 0, 1, 2, 3
QUERY_DTYPE = np.dtype([("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("max_distance", "<f8"), ("shape", "<u4"),
                        ("ignore_body", "<u4"), ("mask", "<u4"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("index_a", "<u4"), ("index_b", "<u4"), ("distance", "<f8"),
                      ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,)), ("normal", "<f8", (3,))])
INF = float("inf")


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


class Shape:
    """A polytope of the table as the candidate lists read it."""

    def __init__(self, poly):
        self.verts = np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3)
        self.planes = rm.polytope_planes(poly)
        self.edges = np.asarray(poly["edges"], dtype=np.int64).reshape(-1, 2)
        fo, fi = np.asarray(poly["face_offsets"]), np.asarray(poly["face_indices"])
        self.faces = [[int(x) for x in fi[fo[f]:fo[f + 1]]] for f in range(len(fo) - 1)]
        self.centroid = tuple(float(x) for x in poly["centroid"])
        self.radius = om.shape_radius(poly)
        # "x lies in face F": per face the (a, side) of every edge, side already turned away from the face's third vertex
        self.sides = []
        for f, idx in enumerate(self.faces):
            n = tuple(float(x) for x in self.planes[f, :3])
            m, rows = len(idx), []
            for k in range(m):
                a, b, c = (tuple(float(x) for x in self.verts[idx[(k + j) % m]]) for j in range(3))
                side = rm.cross(sub(b, a), n)
                if rm.dot(side, sub(c, a)) > 0.0:
                    side = (-side[0], -side[1], -side[2])
                rows.append((a, side))
            self.sides.append(rows)


class PointShape:
    """The point volume: one vertex, no faces, one edge from the vertex to itself."""
    verts = np.zeros((1, 3))
    planes = np.zeros((0, 4))
    edges = np.zeros((1, 2), dtype=np.int64)
    faces, sides = [], []
    radius = 0.0


def vertex_face(p, S):
    """d2 (V, F) of the vertices p (3 columns of V, in S's local space) over the faces of S (+inf: the candidate does not count), and
    the feet, a list per face of 3 columns."""
    V, F = len(p[0]), len(S.planes)
    d2 = np.full((V, F), INF)
    feet = []
    with np.errstate(all="ignore"):
        for f in range(F):
            n, disp = tuple(float(x) for x in S.planes[f, :3]), float(S.planes[f, 3])
            h = rm.dot(n, p) - disp
            foot = (p[0] - h * n[0], p[1] - h * n[1], p[2] - h * n[2])
            ok = h >= 0.0
            for a, side in S.sides[f]:
                ok = ok & (rm.dot(side, sub(foot, a)) <= 0.0)
            d2[:, f] = np.where(ok, h * h, INF)
            feet.append(foot)
    return d2, feet


def clamp(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def segments(p0, p1, q0, q1):
    """Clamped closest points of the segments p0 p1 (3 columns (EA, 1)) and q0 q1 ((1, EB)): d2 (EA, EB), s, t."""
    with np.errstate(all="ignore"):
        u, w, r = sub(p1, p0), sub(q1, q0), sub(p0, q0)
        a, e, f = rm.dot(u, u), rm.dot(w, w), rm.dot(w, r)
        c, b = rm.dot(u, r), rm.dot(u, w)
        den = a * e - b * b
        s = np.where(den > 0.0, clamp((b * f - c * e) / den), 0.0)
        t = (b * s + f) / e
        s = np.where(t < 0.0, clamp((-c) / a), np.where(t > 1.0, clamp((b - c) / a), s))
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        s = np.where(e == 0.0, clamp((-c) / a), s)                          # e == 0 (a != 0): t = 0
        t = np.where(e == 0.0, 0.0, t)
        t = np.where(a == 0.0, clamp(f / e), t)                             # a == 0 (e != 0): s = 0
        s = np.where(a == 0.0, 0.0, s)
        t = np.where((a == 0.0) & (e == 0.0), 0.0, t)
        s, t = np.broadcast_to(s, den.shape), np.broadcast_to(t, den.shape)
        ca = tuple(p0[k] + u[k] * s for k in range(3))
        cb = tuple(q0[k] + w[k] * t for k in range(3))
        g = sub(ca, cb)
        d2 = rm.dot(g, g)
    return np.where(np.isnan(d2), INF, d2), ca, cb


class Scene:
    """The bodies' side of the model, computed once and shared by the queries of a test."""

    def __init__(self, bodies, shape_id, polytopes, groups=None):
        self.ov = om.Scene(bodies, shape_id, polytopes, groups)             # the oracle's frames, centres and op_sat
        self.shapes = [Shape(p) for p in polytopes]
        self.sid = [int(x) for x in shape_id]
        origin, rot = rm.body_frames(bodies)
        n = len(self.sid)
        self.pos = [tuple(float(origin[a, i]) for a in range(3)) for i in range(n)]
        self.rot = [tuple(float(rot[a, i]) for a in range(4)) for i in range(n)]
        self.centres = np.array([frame_mul(self.pos[i], self.rot[i], self.shapes[s].centroid) for i, s in enumerate(self.sid)]).reshape(-1, 3)
        self.finite = np.isfinite(origin).all(axis=0) & np.isfinite(rot).all(axis=0) & np.isfinite(self.centres).all(axis=1)
        self.body_radius = np.array([self.shapes[s].radius for s in self.sid])
        self.groups = None if groups is None else [int(g) for g in groups]
        self._world = {}

    def body_world(self, i):
        if i not in self._world:
            bw = frame_mul(self.pos[i], self.rot[i], cols(self.shapes[self.sid[i]].verts))
            self._world[i] = (bw, frame_inverse(self.pos[i], self.rot[i]))
        return self._world[i]

    def volume(self, q):
        """The query's side of every pair, or None for a query that finds nothing."""
        sq = int(q["shape"])
        point = sq == POINT
        if not point and sq >= len(self.shapes):
            return None
        pos = tuple(float(x) for x in q["position"])
        rot = tuple(float(x) for x in q["rotation"])
        dmax = float(q["max_distance"])
        if not all(math.isfinite(x) for x in pos + rot) or not dmax >= 0.0:
            return None
        A = PointShape if point else self.shapes[sq]
        centre = pos if point else frame_mul(pos, rot, A.centroid)
        if not all(math.isfinite(x) for x in centre):
            return None
        ip, qi = frame_inverse(pos, rot)
        aw = tuple(np.array([x]) for x in pos) if point else frame_mul(pos, rot, cols(A.verts))
        return {"shape": A, "sq": sq, "point": point, "pos": pos, "rot": rot, "dmax": dmax, "aw": aw, "ip": ip, "qi": qi,
                "centre": tuple(float(x) for x in centre), "frame": ob.frame(q["position"], q["rotation"])}

    def overlaps(self, vol, i, a_in_b):
        """Step 1: rules 2 and 3 of the overlap query (the point volume: radius 0, then the deepest face plane)."""
        cb, cq = self.ov.centres[i], vol["centre"]
        between = (float(cb[0]) - cq[0], float(cb[1]) - cq[1], float(cb[2]) - cq[2])
        reach = vol["shape"].radius + self.body_radius[i]
        if not (between[0] * between[0] + between[1] * between[1] + between[2] * between[2] < reach * reach):
            return False
        B = self.shapes[self.sid[i]]
        if vol["point"]:
            p = (a_in_b[0][0], a_in_b[1][0], a_in_b[2][0])
            deepest = first_max([np.float64(rm.dot(tuple(B.planes[f, :3]), p) - B.planes[f, 3]) for f in range(len(B.planes))])
            return bool(deepest < 0.0)
        m = ob.Manifold()
        self.ov.L.op_sat(vol["frame"], self.ov.frames[i], C.byref(self.ov.polys[vol["sq"]]), C.byref(self.ov.polys[self.sid[i]]), C.byref(m))
        return not m.separated

    def pair(self, vol, i):
        """One (volume, body) pair: None (no answer at all) or (distance, feature, index_a, index_b, point_a, point_b)."""
        A, B = vol["shape"], self.shapes[self.sid[i]]
        bw, (ipb, qib) = self.body_world(i)
        aw = vol["aw"]
        a_in_b = frame_mul(ipb, qib, aw)
        if self.overlaps(vol, i, a_in_b):
            return (0.0, OVERLAP, NO_HIT, NO_HIT, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        best, what = INF, None
        # (a) vertices of the volume over faces of the body, in the body's space
        d2, feet = vertex_face(a_in_b, B)
        if d2.size and d2.min() < best:
            best = float(d2.min())
            v, f = divmod(int(np.argmin(d2)), len(B.planes))               # the first minimum in v * n_faces_b + f
            what = ("a", v, f, tuple(float(feet[f][k][v]) for k in range(3)))
        # (b) vertices of the body over faces of the volume, in the volume's space
        if len(A.planes):
            b_in_a = frame_mul(vol["ip"], vol["qi"], bw)
            d2, feet = vertex_face(b_in_a, A)
            if d2.min() < best:
                best = float(d2.min())
                v, f = divmod(int(np.argmin(d2)), len(A.planes))
                what = ("b", v, f, tuple(float(feet[f][k][v]) for k in range(3)))
        # (c) edges of the volume against edges of the body, in world space
        ea, eb = A.edges, B.edges
        p0, p1 = tuple(aw[k][ea[:, 0]][:, None] for k in range(3)), tuple(aw[k][ea[:, 1]][:, None] for k in range(3))
        q0, q1 = tuple(bw[k][eb[:, 0]][None, :] for k in range(3)), tuple(bw[k][eb[:, 1]][None, :] for k in range(3))
        d2, ca, cb = segments(p0, p1, q0, q1)
        if d2.size and d2.min() < best:
            best = float(d2.min())
            i_a, j_b = divmod(int(np.argmin(d2)), len(eb))
            what = ("c", i_a, j_b, None)
        if what is None:
            return None
        kind, x, y, foot = what
        if kind == "a":
            pa = tuple(float(aw[k][x]) for k in range(3))
            pb = tuple(float(c) for c in frame_mul(self.pos[i], self.rot[i], foot))
            feature, ia, ib = FEATURE_FACE_B, x, y
        elif kind == "b":
            pb = tuple(float(bw[k][x]) for k in range(3))
            pa = tuple(float(c) for c in frame_mul(vol["pos"], vol["rot"], foot))
            feature, ia, ib = FEATURE_FACE_A, y, x
        else:
            pa = tuple(float(np.broadcast_to(ca[k], d2.shape)[x, y]) for k in range(3))
            pb = tuple(float(np.broadcast_to(cb[k], d2.shape)[x, y]) for k in range(3))
            feature, ia, ib = FEATURE_EDGES, x, y
        return (math.sqrt(best), feature, ia, ib, pa, pb)

    def query_one(self, q, masked=False):
        """(body, pair result) of one query record; body None: nothing found."""
        vol = self.volume(q)
        if vol is None:
            return None, None
        # candidates, nearest first by a LOWER bound of the distance: the gap between the bounding spheres (0.1 % larger).  A
        # body whose bound lies beyond the best distance cannot win.  This only saves work; every decision is pair()'s.
        with np.errstate(all="ignore"):
            w = self.centres - np.array(vol["centre"])
            gap = np.sqrt((w * w).sum(axis=1)) - (vol["shape"].radius + self.body_radius) * 1.001 - 1e-9
            bound = np.where(gap > 0.0, gap * (1.0 - 1e-9), 0.0)
            bound = np.where(self.finite & ~np.isnan(bound) & (bound <= vol["dmax"]), bound, INF)
        ignore, mask = int(q["ignore_body"]), int(q["mask"])
        best_body, best = None, None
        for i in np.argsort(bound, kind="stable"):
            i = int(i)
            if bound[i] == INF or (best is not None and bound[i] > best[0]):
                break
            if i == ignore:
                continue
            if masked and ((0xFFFFFFFF if self.groups is None else self.groups[i]) & mask) == 0:
                continue
            got = self.pair(vol, i)
            if got is None or not got[0] <= vol["dmax"]:
                continue
            if best is None or got[0] < best[0] or (got[0] == best[0] and i < best_body):
                best_body, best = i, got
        return best_body, best

    def distance(self, queries, masked=False):
        """HIT_DTYPE records as the library returns them."""
        queries = np.asarray(queries).reshape(-1)
        out = np.zeros(len(queries), dtype=HIT_DTYPE)
        out["body"], out["index_a"], out["index_b"], out["distance"] = NO_HIT, NO_HIT, NO_HIT, INF
        for k, q in enumerate(queries):
            body, got = self.query_one(q, masked)
            if body is None:
                continue
            d, feature, ia, ib, pa, pb = got
            out["body"][k], out["feature"][k], out["index_a"][k], out["index_b"][k], out["distance"][k] = body, feature, ia, ib, d
            out["point_a"][k], out["point_b"][k] = pa, pb
            if d != 0.0:
                inv = 1.0 / d
                out["normal"][k] = [(pa[a] - pb[a]) * inv for a in range(3)]
        return out


def one(position, rotation=(1.0, 0.0, 0.0, 0.0), shape=POINT, max_distance=INF, ignore=NO_HIT, mask=0xFFFFFFFF):
    q = np.zeros(1, dtype=QUERY_DTYPE)
    q["position"], q["rotation"], q["max_distance"], q["shape"], q["ignore_body"], q["mask"] = position, rotation, max_distance, shape, ignore, mask
    return q


def distance(bodies, shape_id, polytopes, queries, masked=False, groups=None):
    return Scene(bodies, shape_id, polytopes, groups).distance(queries, masked)
