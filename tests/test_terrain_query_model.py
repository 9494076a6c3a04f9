"""The terrain query model's own checks (tests/terrain_query_model.py), CPU only: its planes are terrain_model's; analytic
distances on a flat and on a tilted field; downward rays through interior points, grid lines, corners and the diagonals never
leak; the hit point lies on the surface sample() reports; the vertex sweep and the vertex overlap on a flat field; the census of
the random rays the GPU tests use."""
import math

import numpy as np

import raycast_model as rm
import terrain_model as tm
import terrain_query_model as tq

INF = math.inf
# |hit.z - sample(hit.x, hit.y)| over the downward rays of test_hit_points_lie_on_the_sampled_surface, measured with this model
# (1 523 rays from z = 3 in all, none leaks; the 1 200 of them on the recipe's field, heights up to 0.6, whose (x, y) sample() places
# inside the field are compared): the largest is 8.33e-16; the test asserts 16 times it.
SURFACE_ERROR = 8.33e-16


def recipe():
    return tm.Terrain(tq.recipe_heights(), tq.RECIPE_ORIGIN, tq.RECIPE_CELL)


def probe_xy(field, rng, per_cell=6):
    """Points inside the field's closed box: interior points of both triangles, on grid lines, at corners, on the diagonals."""
    xs = [field.x0 + i * field.dx for i in range(field.nx)]
    ys = [field.y0 + j * field.dy for j in range(field.ny)]
    pts = [(x, y) for x in xs for y in ys]
    for i in range(field.nx - 1):
        for j in range(field.ny - 1):
            for _ in range(per_cell):
                a, b = rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0)
                pts.append((xs[i] + a * field.dx, ys[j] + b * field.dy))
                pts.append((xs[i] + a * field.dx, ys[j]))                       # on a grid line along x
                pts.append((xs[i], ys[j] + b * field.dy))                       # ... along y
                pts.append((xs[i] + a * field.dx, ys[j] + a * field.dy))        # on (or within rounding of) the diagonal
    return [(x, y) for x, y in pts if xs[0] <= x <= xs[-1] and ys[0] <= y <= ys[-1]]


def test_planes_equal_terrain_models_for_every_triangle():
    field = tm.Terrain(tm.bumpy_field(9, 7, 4), (-3.1, -2.3), (0.7, 0.9))
    seen = 0
    for j in range(field.ny - 1):
        for i in range(field.nx - 1):
            for k, (a, b) in enumerate(((0.7, 0.2), (0.2, 0.7))):
                x = (field.x0 + (i + a) * field.dx, field.y0 + (j + b) * field.dy, 0.0)
                assert tq.triangle_plane(field, i, j, k) == field.plane(x)
                seen += 1
    assert seen == 96


def test_flat_field_at_binary_spacing_gives_exact_distances():
    field = tm.Terrain(np.full((4, 5), 0.25), (-1.0, 2.0), (0.5, 0.25))
    assert tq.raycast(field, (-0.375, 2.3125, 2.0), (0.0, 0.0, -1.0), INF) == (1.75, tq.triangle_number(field, 1, 1, 0))
    assert tq.raycast(field, (-0.375, 2.3125, 2.0), (0.0, 0.0, -2.0), INF)[0] == 0.875
    assert tq.raycast(field, (-0.375, 2.3125, 2.0), (0.0, 0.0, -1.0), 1.5) is None                 # too short
    assert tq.raycast(field, (-0.375, 2.3125, 2.0), (0.0, 0.0, 1.0), INF) is None                  # pointing up
    assert tq.raycast(field, (-0.375, 2.3125, 0.0), (0.0, 0.0, 1.0), INF) == (0.0, tq.triangle_number(field, 1, 1, 0))   # from inside
    assert tq.raycast(field, (-2.0, 2.3125, 2.0), (0.0, 0.0, -1.0), INF) is None                   # beside the field
    # from outside through the outer wall, below the surface: the wall x = -1 is met at t = 1
    assert tq.raycast(field, (-2.0, 2.3125, 0.0), (1.0, 0.0, 0.0), INF) == (1.0, tq.triangle_number(field, 0, 1, 1))
    # a slanted ray onto the plane z = 0.25: (2 - 0.25) / 1 = 1.75 along (0.25, 0, -1)
    t, _ = tq.raycast(field, (-0.75, 2.3125, 2.0), (0.25, 0.0, -1.0), INF)
    assert t == 1.75


def test_tilted_plane_gives_the_analytic_distance():
    """A field sampled from h = 0.3 x - 0.2 y: a ray o + t dir meets it at t = (h(o) - o.z) / (dir.z - 0.3 dir.x + 0.2 dir.y).
    The model's t goes through about ten roundings of numbers up to |o| <= 5 (the unit normal, two dot products, one
    division): 5 * 10 * 2^-53 = 5.6e-15 bounds its error; the analytic value is rounded likewise."""
    origin, cell = (-3.0, -2.0), (0.7, 0.9)
    field = tm.Terrain(tm.tilted_field(9, 7, origin, cell, 0.3, -0.2), origin, cell)
    import random
    rng = random.Random(3)
    worst = hits = 0
    for _ in range(400):
        o = (rng.uniform(-2.9, 2.5), rng.uniform(-1.9, 3.3), rng.uniform(2.0, 4.0))
        d = (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1.0)
        want = (0.3 * o[0] - 0.2 * o[1] - o[2]) / (d[2] - 0.3 * d[0] + 0.2 * d[1])
        x, y = o[0] + want * d[0], o[1] + want * d[1]
        if not (-3.0 < x < 2.6 and -2.0 < y < 3.4):
            continue
        got = tq.raycast(field, o, d, INF)
        assert got is not None
        worst = max(worst, abs(got[0] - want))
        hits += 1
    print("%d rays, largest |t - analytic| %.3g" % (hits, worst))
    assert hits > 300 and worst <= 1.2e-14


def test_downward_rays_never_leak_and_hit_points_lie_on_the_sampled_surface():
    import random
    rng = random.Random(5)
    worst = count = compared = 0
    for field in (recipe(), tm.Terrain(tm.bumpy_field(5, 4, 2), (-1.0, 2.0), (0.5, 0.25))):
        for x, y in probe_xy(field, rng):
            hit = tq.raycast(field, (x, y, 3.0), (0.0, 0.0, -1.0), INF)
            assert hit is not None, (x, y)
            count += 1
            if field.H[0][0] == tq.recipe_heights()[0][0]:
                z, surface = 3.0 + (-1.0) * hit[0], field.sample(x, y)[0]
                if surface == surface:                                          # (NaN: the far edges, where sample() is outside)
                    worst = max(worst, abs(z - surface))
                    compared += 1
    print("%d downward rays, none leaked; %d compared with sample(): largest |z - sample| %.3g" % (count, compared, worst))
    assert count > 1000 and compared > 500
    assert worst <= 16.0 * SURFACE_ERROR


def test_vertex_sweep_and_vertex_overlap_on_a_flat_field():
    field = tm.Terrain(np.full((4, 5), 0.25), (-1.0, 2.0), (0.5, 0.25))
    polys = [rm.box((0.0, 0.0, 0.0), (0.25, 0.125, 0.5))]
    sweeps = np.zeros(3, dtype=[("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("direction", "<f8", (3,)), ("max_distance", "<f8"),
                                ("shape", "<u4"), ("ignore_body", "<u4"), ("mask", "<u4"), ("reserved", "<u4")])
    sweeps["rotation"] = (1.0, 0.0, 0.0, 0.0)
    sweeps["direction"], sweeps["max_distance"] = (0.0, 0.0, -1.0), INF
    sweeps["position"] = [(-0.5, 2.25, 1.0), (-0.5, 2.25, 0.0), (-3.0, 2.25, 1.0)]           # above, in the ground, beside the field
    hits = tq.sweep_hits(field, polys, sweeps)
    assert hits["body"].tolist() == [tq.HIT_TERRAIN, tq.HIT_TERRAIN, tq.NO_HIT]
    assert hits["distance"][0] == 0.75 and hits["feature"][0] == tq.FEATURE_FACE_B and hits["position"][0].tolist() == [-0.5, 2.25, 0.25]
    assert hits["normal"][0].tolist() == [0.0, 0.0, 1.0]
    assert hits["distance"][1] == 0.0 and hits["feature"][1] == tq.SWEEP_INITIAL and hits["face"][1] == tq.NO_HIT
    identity = (1.0, 0.0, 0.0, 0.0)
    assert tq.overlap_entry(field, polys[0], (-0.5, 2.25, 0.125), identity) == -0.125
    assert tq.overlap_entry(field, polys[0], (-0.5, 2.25, 0.25), identity) is None                # touching is free: s = 0
    assert tq.overlap_entry(field, polys[0], (-3.0, 2.25, 0.0), identity) is None                 # beside the field


def test_the_random_rays_of_the_gpu_test_cover_every_class():
    """The recipe of tests/test_gpu_terrain_queries.py: each of top hits, wall or diagonal hits, inside and misses is at least
    3 % of 6000 rays."""
    field = recipe()
    from constraint_solver_amd import capi
    rays = capi.rays(*tq.random_rays(6000, 1)[:2], tq.random_rays(6000, 1)[2])
    census = tq.classify(field, rays, tq.ray_hits(field, rays))
    print("top %d, wall or diagonal %d, inside %d, miss %d" % census)
    assert sum(census) == 6000 and min(census) >= 180
