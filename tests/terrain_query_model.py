"""Independent model of the TERRAIN in the scene queries (include/xpbd.h, "Terrain in the scene queries"), in plain Python floats:
the definition itself, brute force over all triangles.  The planes are terrain_model.Terrain's formulas (steps 4 to 6 of the
header's lookup) evaluated for a triangle by its number instead of through a point; tests/test_terrain_query_model.py checks that
the two agree for every triangle.  Python never fuses a multiply-add and its division is the correctly rounded one, so every t
here is what an f64 evaluation of the header's rule in the header's order gives.

  ray_triangle      one ray against the prism under one triangle
  raycast           the terrain's answer for one ray: the minimum over all triangles under (t, triangle)
  ray_hits          ... for RAY_DTYPE records, as RAY_HIT_DTYPE-shaped records; merge_ray_hits puts them next to raycast_model's
  sweep_hits        every world vertex of the volume as a ray; the minimum under (t, triangle, vertex)
  overlap_entry     the stepper's lookup at every vertex: the smallest negative s, or None"""
import math

import numpy as np

import raycast_model as rm
from material_model import dot, magnitude, scale

INF = math.inf
NO_HIT = RAY_INSIDE = 0xFFFFFFFF
HIT_TERRAIN = 0xFFFFFFFE
QUERY_TERRAIN = 0x100
FEATURE_FACE_B, SWEEP_INITIAL = 1, 3

RAY_HIT_DTYPE = np.dtype([("body", "<u4"), ("face", "<u4"), ("distance", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,))])
SWEEP_HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("face", "<u4"), ("reserved", "<u4"), ("distance", "<f8"),
                            ("position", "<f8", (3,)), ("normal", "<f8", (3,))])


def triangle_number(terrain, i, j, k):
    return 2 * (j * (terrain.nx - 1) + i) + k


def triangle_plane(terrain, i, j, k):
    """(n, d) of triangle (i, j, k): steps 4 to 6 of the lookup with fi = i, fj = j and the triangle given."""
    H = terrain.H
    h00, h10, h01, h11 = H[j][i], H[j][i + 1], H[j + 1][i], H[j + 1][i + 1]
    if k == 0:
        sx, sy = (h10 - h00) / terrain.dx, (h11 - h10) / terrain.dy
    else:
        sx, sy = (h11 - h01) / terrain.dx, (h01 - h00) / terrain.dy
    raw = (-sx, -sy, 1.0)
    n = scale(raw, 1.0 / magnitude(raw))
    d = dot(n, (terrain.x0 + float(i) * terrain.dx, terrain.y0 + float(j) * terrain.dy, h00))
    return n, d


def planes_of(terrain):
    """{(i, j, k): (n, d)} of every triangle, cached on the terrain."""
    table = getattr(terrain, "_query_planes", None)
    if table is None:
        table = {(i, j, k): triangle_plane(terrain, i, j, k) for j in range(terrain.ny - 1) for i in range(terrain.nx - 1) for k in (0, 1)}
        terrain._query_planes = table
    return table


def ray_valid(o, d, tmax):
    finite = all(math.isfinite(x) for x in o) and all(math.isfinite(x) for x in d)
    return finite and any(x != 0.0 for x in d) and tmax >= 0.0


def ray_triangle(terrain, i, j, k, o, d, tmax, plane=None):
    """t of the ray against the prism under triangle (i, j, k), or None: the header's rule, constraint by constraint."""
    n, disp = plane if plane is not None else triangle_plane(terrain, i, j, k)
    state = [0.0, tmax]                                         # t_lo, t_hi

    def constraint(s, v):                                       # False: the ray misses
        if s != s or v != v:
            return False
        if v < 0.0:
            tk = (-s) / v
            if tk > state[0]:
                state[0] = tk
        elif v > 0.0:
            tk = (-s) / v
            if tk < state[1]:
                state[1] = tk
        elif s > 0.0:
            return False
        return True

    def slab(lo, hi, oa, da):
        if da == 0.0:
            return lo <= oa <= hi
        t1, t2 = (lo - oa) / da, (hi - oa) / da
        tn, tf = (t1, t2) if t1 < t2 else (t2, t1)
        if tn > state[0]:
            state[0] = tn
        if tf < state[1]:
            state[1] = tf
        return True

    xi, xi1 = terrain.x0 + float(i) * terrain.dx, terrain.x0 + float(i + 1) * terrain.dx
    yj, yj1 = terrain.y0 + float(j) * terrain.dy, terrain.y0 + float(j + 1) * terrain.dy
    if not constraint(dot(n, o) - disp, dot(n, d)):
        return None
    if not slab(xi, xi1, o[0], d[0]) or not slab(yj, yj1, o[1], d[1]):
        return None
    g = (o[0] - xi) * terrain.dy - (o[1] - yj) * terrain.dx
    gv = d[0] * terrain.dy - d[1] * terrain.dx
    if not (constraint(g, gv) if k == 1 else constraint(-g, -gv)):
        return None
    return state[0] if state[0] <= state[1] else None


def raycast(terrain, o, d, tmax):
    """(t, triangle number) of the terrain's answer, or None: the minimum over every triangle under (t, number)."""
    o, d, tmax = tuple(float(x) for x in o), tuple(float(x) for x in d), float(tmax)
    if not ray_valid(o, d, tmax):
        return None
    best = None
    for (i, j, k), plane in planes_of(terrain).items():
        t = ray_triangle(terrain, i, j, k, o, d, tmax, plane)
        if t is not None:
            cand = (t, triangle_number(terrain, i, j, k))
            if best is None or cand < best:
                best = cand
    return best


def triangle_of_number(terrain, number):
    cell, k = divmod(number, 2)
    j, i = divmod(cell, terrain.nx - 1)
    return i, j, k


def ray_hits(terrain, rays):
    """RAY_HIT_DTYPE-shaped records of the terrain alone for RAY_DTYPE records (a miss: {NO_HIT, NO_HIT, inf, 0, 0})."""
    out = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
    out["body"], out["face"], out["distance"] = NO_HIT, NO_HIT, INF
    for r, ray in enumerate(rays):
        o, d = tuple(float(x) for x in ray["origin"]), tuple(float(x) for x in ray["direction"])
        hit = raycast(terrain, o, d, float(ray["max_distance"]))
        if hit is None:
            continue
        t, number = hit
        out["body"][r], out["distance"][r] = HIT_TERRAIN, t
        out["point"][r] = [o[a] + d[a] * t for a in range(3)]
        if t > 0.0:                                             # something entered
            out["face"][r] = number
            out["normal"][r] = planes_of(terrain)[triangle_of_number(terrain, number)][0]
        else:
            out["face"][r] = RAY_INSIDE
    return out


def body_ray_hits(model_hits):
    """raycast_model.raycast's dict as RAY_HIT_DTYPE-shaped records."""
    out = np.zeros(len(model_hits["body"]), dtype=RAY_HIT_DTYPE)
    for name in RAY_HIT_DTYPE.names:
        out[name] = model_hits[name]
    return out


def merge_ray_hits(bodies, terrain_hits):
    """Per ray the smaller of the two answers under (t, body): a body wins a tie against the terrain."""
    out = bodies.copy()
    for r in range(len(out)):
        a, b = (float(bodies["distance"][r]), int(bodies["body"][r])), (float(terrain_hits["distance"][r]), int(terrain_hits["body"][r]))
        if b < a:
            out[r] = terrain_hits[r]
    return out


def world_vertices(poly, position, rotation):
    """fa * a_v of every vertex: rotation * v + position in cgmath's order (raycast_model.rotate)."""
    q, p = tuple(float(x) for x in rotation), tuple(float(x) for x in position)
    out = []
    for v in np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3):
        r = rm.rotate(q, tuple(float(x) for x in v))
        out.append((r[0] + p[0], r[1] + p[1], r[2] + p[2]))
    return out


def sweep_terrain(terrain, polytopes, sweep):
    """(t, triangle number, vertex) of one SWEEP_DTYPE record against the terrain, or None."""
    shape = int(sweep["shape"])
    pos, rot = tuple(float(x) for x in sweep["position"]), tuple(float(x) for x in sweep["rotation"])
    d, tmax = tuple(float(x) for x in sweep["direction"]), float(sweep["max_distance"])
    if shape >= len(polytopes) or not ray_valid(pos, d, tmax) or not all(math.isfinite(x) for x in rot):
        return None
    best = None
    for v, x in enumerate(world_vertices(polytopes[shape], pos, rot)):
        hit = raycast(terrain, x, d, tmax)
        if hit is not None and (best is None or hit + (v,) < best):
            best = hit + (v,)
    return best


def sweep_hits(terrain, polytopes, sweeps, body_hits=None):
    """SWEEP_HIT_DTYPE records: the terrain's answer where it is strictly earlier than body_hits' (None: misses), else those."""
    out = np.zeros(len(sweeps), dtype=SWEEP_HIT_DTYPE)
    if body_hits is None:
        out["body"], out["face"], out["distance"] = NO_HIT, NO_HIT, INF
    else:
        for name in SWEEP_HIT_DTYPE.names:
            out[name] = body_hits[name]
    for q, sweep in enumerate(sweeps):
        best = sweep_terrain(terrain, polytopes, sweep)
        if best is None or not best[0] < float(out["distance"][q]):
            continue
        t, number, _ = best
        h = out[q]
        h["body"], h["reserved"], h["distance"] = HIT_TERRAIN, 0, t
        h["position"] = [float(sweep["position"][a]) + float(sweep["direction"][a]) * t for a in range(3)]
        if t > 0.0:
            h["feature"], h["face"] = FEATURE_FACE_B, number
            h["normal"] = planes_of(terrain)[triangle_of_number(terrain, number)][0]
        else:
            h["feature"], h["face"], h["normal"] = SWEEP_INITIAL, NO_HIT, 0.0
    return out


def overlap_entry(terrain, poly, position, rotation):
    """The separation of the terrain's entry for a volume -- the smallest s < 0 over its vertices by the stepper's lookup, the
    first minimum -- or None when no vertex is under the ground inside the field."""
    lowest = None
    for x in world_vertices(poly, position, rotation):
        plane = terrain.plane(x)
        if plane is None:
            continue
        s = dot(plane[0], x) - plane[1]
        if s < 0.0 and (lowest is None or s < lowest):
            lowest = s
    return lowest


# ---- fields and rays of the tests (CPU model and GPU alike) -----------------------------------------------------------------
RECIPE_ORIGIN, RECIPE_CELL = (-3.1, -2.3), (0.7, 0.9)


def recipe_heights(nx=9, ny=7):
    return np.array([[0.6 * math.sin(0.9 * i + 0.3) * math.cos(0.7 * j) for i in range(nx)] for j in range(ny)])


def random_rays(n, seed):
    """(origins, directions, max_distance): origins uniform in [-5, 5]^2 x [-1, 4], directions gauss(0, 1)^3 with 0.5 taken off z,
    max_distance drawn from {inf, 3, 10}."""
    import random
    rng = random.Random(seed)
    o = np.array([[rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0), rng.uniform(-1.0, 4.0)] for _ in range(n)])
    d = np.array([[rng.gauss(0.0, 1.0), rng.gauss(0.0, 1.0), rng.gauss(0.0, 1.0) - 0.5] for _ in range(n)])
    m = np.array([rng.choice((INF, 3.0, 10.0)) for _ in range(n)])
    return o, d, m


def classify(terrain, rays, hits):
    """How many rays hit through the top plane, through a wall or the diagonal, start inside, and miss."""
    top = side = inside = miss = 0
    for ray, h in zip(rays, hits):
        if h["body"] != HIT_TERRAIN:
            miss += 1
        elif h["face"] == RAY_INSIDE:
            inside += 1
        else:
            n, disp = planes_of(terrain)[triangle_of_number(terrain, int(h["face"]))]
            o, d = tuple(float(x) for x in ray["origin"]), tuple(float(x) for x in ray["direction"])
            v = dot(n, d)
            if v < 0.0 and (-(dot(n, o) - disp)) / v == h["distance"]:
                top += 1
            else:
                side += 1
    return top, side, inside, miss
