"""Independent f64 model of the terrain distance queries (include/xpbd.h, "Terrain in the distance queries"): every query against
EVERY feature of the heightfield's surface on the CPU -- all triangles, all samples, all terrain edges, no walk.

Written from the header's text.  The triangles' planes come from terrain_model.Terrain's formulas (TERRAIN, steps 4 to 6), rule
1 (i) is terrain_model.Terrain.plane itself, rule 1 (ii) is the ray-body rule restated here, and rules 2 (b) and 2 (c) are the
distance model's own vertex_face and segments (tests/distance_model.py), as the header says they are.  The candidates of a class
are laid out terrain feature first and the volume's index second, so numpy's argmin -- the first minimum of the flattened array
-- is the first minimum of the header's literal loop, and the classes are visited (a), (b), (c) with "strictly smaller".  numpy
never fuses a multiply-add, and its / and sqrt are correctly rounded.  Nothing here shares code with the library.

Polytopes are dicts as capi.World.set_polytopes takes them; queries are records with the fields of distance_model.QUERY_DTYPE."""
import math

import numpy as np

import distance_model as dm
import raycast_model as rm
from distance_model import FEATURE_EDGES, FEATURE_FACE_A, FEATURE_FACE_B, HIT_DTYPE, INF, NO_HIT, OVERLAP, POINT, QUERY_DTYPE, sub
from material_model import magnitude, scale
from sweep_model import cols, frame_inverse, frame_mul

HIT_TERRAIN = 0xFFFFFFFE


class Surface:
    """The features of a terrain_model.Terrain, each with its number."""

    def __init__(self, terrain):
        t = self.terrain = terrain
        nx, ny = t.nx, t.ny
        self.nx, self.ny = nx, ny
        # samples, number j * nx + i
        self.P = (np.array([t.x0 + float(i) * t.dx for j in range(ny) for i in range(nx)]),
                  np.array([t.y0 + float(j) * t.dy for j in range(ny) for i in range(nx)]),
                  np.array([t.H[j][i] for j in range(ny) for i in range(nx)]))
        # triangles, number 2 * (j * (nx - 1) + i) + k: the plane by steps 4 to 6 and the borders of the prism
        rows = []
        for j in range(ny - 1):
            for i in range(nx - 1):
                h00, h10, h01, h11 = t.H[j][i], t.H[j][i + 1], t.H[j + 1][i], t.H[j + 1][i + 1]
                for k in range(2):
                    if k == 0:
                        sx, sy = (h10 - h00) / t.dx, (h11 - h10) / t.dy
                    else:
                        sx, sy = (h11 - h01) / t.dx, (h01 - h00) / t.dy
                    raw = (-sx, -sy, 1.0)
                    n = scale(raw, 1.0 / magnitude(raw))
                    d = rm.dot(n, (t.x0 + float(i) * t.dx, t.y0 + float(j) * t.dy, h00))
                    rows.append((n[0], n[1], n[2], d, t.x0 + float(i) * t.dx, t.x0 + float(i + 1) * t.dx, t.y0 + float(j) * t.dy,
                                 t.y0 + float(j + 1) * t.dy, float(k)))
        self.tri = np.array(rows).T                                          # (9, T)
        # terrain edges, number 3 * (j * nx + i) + e, only those that exist, ascending
        numbers, ends = [], []
        for j in range(ny):
            for i in range(nx):
                for e, (di, dj) in enumerate(((1, 0), (0, 1), (1, 1))):
                    if i + di < nx and j + dj < ny:
                        numbers.append(3 * (j * nx + i) + e)
                        ends.append((j * nx + i, (j + dj) * nx + i + di))
        self.edge_number = np.array(numbers)
        ends = np.array(ends)
        self.Q0 = tuple(c[ends[:, 0]] for c in self.P)
        self.Q1 = tuple(c[ends[:, 1]] for c in self.P)


def volume_of(q, shapes):
    """The query's side, or None for a query that finds nothing (distance_model.Scene.volume without the bodies)."""
    sq = int(q["shape"])
    point = sq == POINT
    if not point and sq >= len(shapes):
        return None
    pos = tuple(float(x) for x in q["position"])
    rot = tuple(float(x) for x in q["rotation"])
    dmax = float(q["max_distance"])
    if not all(math.isfinite(x) for x in pos + rot) or not dmax >= 0.0:
        return None
    A = dm.PointShape if point else shapes[sq]
    centre = pos if point else frame_mul(pos, rot, A.centroid)
    if not all(math.isfinite(float(x)) for x in centre):
        return None
    ip, qi = frame_inverse(pos, rot)
    aw = tuple(np.array([x]) for x in pos) if point else frame_mul(pos, rot, cols(A.verts))
    return {"shape": A, "point": point, "pos": pos, "rot": rot, "dmax": dmax, "aw": aw, "ip": ip, "qi": qi}


def vertex_under_ground(surface, vol):
    """Rule 1 (i)."""
    aw = vol["aw"]
    for v in range(len(aw[0])):
        x = (float(aw[0][v]), float(aw[1][v]), float(aw[2][v]))
        plane = surface.terrain.plane(x)
        if plane is not None and rm.dot(plane[0], x) - plane[1] < 0.0:
            return True
    return False


def edge_hits_volume(surface, vol):
    """Rule 1 (ii): every terrain edge as the ray (Q0, Q1 - Q0, 1) against the volume as a body with frame fa."""
    A = vol["shape"]
    if vol["point"] or not len(surface.edge_number):
        return False
    with np.errstate(all="ignore"):
        o = frame_mul(vol["ip"], vol["qi"], surface.Q0)
        d = rm.rotate(vol["qi"], sub(surface.Q1, surface.Q0))
        t_lo, t_hi = np.zeros(len(o[0])), np.ones(len(o[0]))
        miss = np.zeros(len(o[0]), dtype=bool)
        for f in range(len(A.planes)):
            n, disp = tuple(float(x) for x in A.planes[f, :3]), float(A.planes[f, 3])
            s, v = rm.dot(n, o) - disp, rm.dot(n, d)
            miss |= np.isnan(s) | np.isnan(v)
            tk = (-s) / v
            t_lo = np.where((v < 0.0) & (tk > t_lo), tk, t_lo)
            t_hi = np.where((v > 0.0) & (tk < t_hi), tk, t_hi)
            miss |= (v == 0.0) & (s > 0.0)
            miss |= t_lo > t_hi                                              # (only grows / only shrinks: a miss for good)
    return bool((~miss & (t_lo <= t_hi)).any())


def separated_minimum(surface, vol):
    """Rule 2: None (no candidate) or (d2, feature, index_a, index_b, point_a, point_b)."""
    A, aw = vol["shape"], vol["aw"]
    best, what = INF, None
    with np.errstate(all="ignore"):
        # (a) every vertex of the volume against every triangle, in world space: (T, V), triangle first
        nx_, ny_, nz_, d, xi, xi1, yj, yj1, upper = (r[:, None] for r in surface.tri)
        p = tuple(c[None, :] for c in aw)
        h = (nx_ * p[0] + ny_ * p[1] + nz_ * p[2]) - d
        foot = (p[0] - h * nx_, p[1] - h * ny_, p[2] - h * nz_)
        t = surface.terrain
        g = (foot[0] - xi) * t.dy - (foot[1] - yj) * t.dx
        ok = (h >= 0.0) & (xi <= foot[0]) & (foot[0] <= xi1) & (yj <= foot[1]) & (foot[1] <= yj1) & np.where(upper == 1.0, g <= 0.0, g >= 0.0)
        d2 = np.where(ok, h * h, INF)
        if d2.size and d2.min() < best:
            best = float(d2.min())
            tri, v = divmod(int(np.argmin(d2)), d2.shape[1])
            what = (FEATURE_FACE_B, v, tri, tuple(float(c[v]) for c in aw), tuple(float(np.broadcast_to(c, d2.shape)[tri, v]) for c in foot))
        # (b) every sample against every face of the volume, in the volume's space: (S, F), sample first
        if len(A.planes):
            local = frame_mul(vol["ip"], vol["qi"], surface.P)
            d2, feet = dm.vertex_face(local, A)
            if d2.min() < best:
                best = float(d2.min())
                s, f = divmod(int(np.argmin(d2)), d2.shape[1])
                pa = frame_mul(vol["pos"], vol["rot"], tuple(float(feet[f][k][s]) for k in range(3)))
                what = (FEATURE_FACE_A, f, s, tuple(float(c) for c in pa), tuple(float(c[s]) for c in surface.P))
        # (c) every edge of the volume against every terrain edge, in world space: (E_terrain, E_volume), terrain edge first
        ea = A.edges
        p0, p1 = tuple(aw[k][ea[:, 0]][None, :] for k in range(3)), tuple(aw[k][ea[:, 1]][None, :] for k in range(3))
        q0, q1 = tuple(c[:, None] for c in surface.Q0), tuple(c[:, None] for c in surface.Q1)
        d2, ca, cb = dm.segments(p0, p1, q0, q1)
        if d2.size and d2.min() < best:
            best = float(d2.min())
            et, ev = divmod(int(np.argmin(d2)), d2.shape[1])
            what = (FEATURE_EDGES, ev, int(surface.edge_number[et]), tuple(float(np.broadcast_to(c, d2.shape)[et, ev]) for c in ca),
                    tuple(float(np.broadcast_to(c, d2.shape)[et, ev]) for c in cb))
    if what is None:
        return None
    return (best,) + what


def query_one(surface, shapes, q):
    """One HIT_DTYPE record's fields, or None for a miss: (feature, index_a, index_b, distance, point_a, point_b)."""
    vol = volume_of(q, shapes)
    if vol is None:
        return None
    if vertex_under_ground(surface, vol) or edge_hits_volume(surface, vol):
        return (OVERLAP, NO_HIT, NO_HIT, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    got = separated_minimum(surface, vol)
    if got is None:
        return None
    d2, feature, ia, ib, pa, pb = got
    distance = math.sqrt(d2)
    if not distance <= vol["dmax"]:
        return None
    return (feature, ia, ib, distance, pa, pb)


def terrain_distance(terrain, polytopes, queries):
    """HIT_DTYPE records as xpbd_world_terrain_distance returns them; terrain: a terrain_model.Terrain or a Surface."""
    surface = terrain if isinstance(terrain, Surface) else Surface(terrain)
    shapes = [dm.Shape(p) for p in polytopes]
    queries = np.asarray(queries).reshape(-1)
    out = np.zeros(len(queries), dtype=HIT_DTYPE)
    out["body"], out["index_a"], out["index_b"], out["distance"] = NO_HIT, NO_HIT, NO_HIT, INF
    for k, q in enumerate(queries):
        got = query_one(surface, shapes, q)
        if got is None:
            continue
        feature, ia, ib, d, pa, pb = got
        out["body"][k], out["feature"][k], out["index_a"][k], out["index_b"][k], out["distance"][k] = HIT_TERRAIN, feature, ia, ib, d
        out["point_a"][k], out["point_b"][k] = pa, pb
        if d != 0.0:
            inv = 1.0 / d
            out["normal"][k] = [(pa[a] - pb[a]) * inv for a in range(3)]
    return out


def merge(bodies_hits, terrain_hits):
    """The world's nearest thing: the smaller distance of the two answers, a body winning a tie (the header's sentence)."""
    take_terrain = terrain_hits["distance"] < bodies_hits["distance"]
    return np.where(take_terrain, terrain_hits, bodies_hits)
