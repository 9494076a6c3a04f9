"""The terrain distance model (tests/terrain_distance_model.py) on its own: known answers at binary spacing, where the arithmetic
is exact (tests/terrain_distance_cases.py), and 300 random unit cubes over a random field against dense sampling of the surface."""
import math

import numpy as np

import raycast_model as rm
import terrain_distance_cases as tc
import terrain_distance_model as tdm
import terrain_model as tm
from terrain_distance_model import FEATURE_EDGES, FEATURE_FACE_A, FEATURE_FACE_B, HIT_TERRAIN, NO_HIT, OVERLAP

CASES = {name: (f, q) for name, f, q in tc.cases()}


def answer(name):
    (heights, origin, cell), q = CASES[name]
    return tdm.terrain_distance(tm.Terrain(heights, origin, cell), tc.polytopes(), q)[0]


def is_miss(h):
    return (h["body"] == NO_HIT and h["feature"] == 0 and h["index_a"] == NO_HIT and h["index_b"] == NO_HIT and h["distance"] == np.inf
            and not h["point_a"].any() and not h["point_b"].any() and not h["normal"].any())


def is_overlap(h):
    return (h["body"] == HIT_TERRAIN and h["feature"] == OVERLAP and h["index_a"] == NO_HIT and h["index_b"] == NO_HIT and h["distance"] == 0.0
            and not h["point_a"].any() and not h["point_b"].any() and not h["normal"].any())


def test_a_point_above_the_interior_of_a_flat_triangle():
    h = answer("point_over_triangle")
    assert h["body"] == HIT_TERRAIN and h["feature"] == FEATURE_FACE_B and h["index_a"] == 0 and h["index_b"] == 0
    assert h["distance"] == 1.0 and list(h["normal"]) == [0.0, 0.0, 1.0]
    assert list(h["point_a"]) == [-0.625, 2.0625, 1.25] and list(h["point_b"]) == [-0.625, 2.0625, 0.25]


def test_on_a_grid_line_two_triangles_tie_and_the_smaller_number_wins():
    h = answer("point_over_grid_line")                                        # over the wall between cells (0, 0) and (1, 0)
    assert h["feature"] == FEATURE_FACE_B and h["index_b"] == 0 and h["distance"] == 1.0           # triangle 0, not triangle 3
    assert list(h["point_b"]) == [-0.5, 2.0625, 0.25] and list(h["normal"]) == [0.0, 0.0, 1.0]


def test_a_point_on_the_surface_is_at_distance_zero_with_a_real_feature():
    h = answer("point_on_surface")
    assert h["body"] == HIT_TERRAIN and h["feature"] == FEATURE_FACE_B and h["index_b"] == 0 and h["distance"] == 0.0
    assert list(h["point_a"]) == list(h["point_b"]) == [-0.625, 2.0625, 0.25] and not h["normal"].any()


def test_a_point_beside_the_field_finds_the_border_edge():
    h = answer("point_beside_field")
    assert h["feature"] == FEATURE_EDGES and h["index_a"] == 0 and h["index_b"] == 1                # edge (0, 0, 1): up the border x = -1
    assert h["distance"] == 1.0 and list(h["point_b"]) == [-1.0, 2.0625, 0.25] and list(h["normal"]) == [-1.0, 0.0, 0.0]


def test_a_point_above_a_roof_ridge_finds_the_ridge():
    h = answer("point_over_ridge")
    assert h["feature"] == FEATURE_EDGES and h["index_b"] == 3 * 1 + 1 and h["distance"] == 1.0     # edge (1, 0, 1)
    assert list(h["point_b"]) == [-0.5, 2.125, 0.5] and list(h["normal"]) == [0.0, 0.0, 1.0]


def test_under_ground_is_overlap_inside_the_field_and_a_border_edge_outside_it():
    assert is_overlap(answer("point_under_ground_inside"))
    h = answer("point_under_ground_outside")
    assert h["feature"] == FEATURE_EDGES and h["index_b"] == 1 and h["distance"] == math.sqrt(2.0)
    assert list(h["point_b"]) == [-1.0, 2.0625, 0.25]


def test_a_cube_flat_above_a_single_peak_finds_the_sample_under_its_face():
    h = answer("cube_over_peak")
    assert h["body"] == HIT_TERRAIN and h["feature"] == FEATURE_FACE_A and h["index_a"] == 0 and h["index_b"] == 1 * 5 + 2
    assert h["distance"] == 0.5 and list(h["point_a"]) == [0.0, 2.25, 1.0] and list(h["point_b"]) == [0.0, 2.25, 0.5]
    assert list(h["normal"]) == [0.0, 0.0, 1.0]


def test_a_cube_edge_on_across_a_rim_finds_two_edge_interiors():
    h = answer("cube_edge_across_rim")
    assert h["feature"] == FEATURE_EDGES and h["index_a"] == 0 and h["index_b"] == 3 * 1 + 1 and h["distance"] == 0.5
    assert list(h["point_a"]) == [-0.5, 2.125, 1.0] and list(h["point_b"]) == [-0.5, 2.125, 0.5]


def test_overlap_through_a_vertex_and_through_a_ridge_between_the_vertices():
    surface = lambda f: tdm.Surface(tm.Terrain(*f))
    shapes = [tdm.dm.Shape(p) for p in tc.polytopes()]
    f, q = CASES["cube_vertex_under_slope"]                                   # one vertex 2^-20 under the slope: rule (i)
    assert is_overlap(answer("cube_vertex_under_slope"))
    assert tdm.vertex_under_ground(surface(f), tdm.volume_of(q[0], shapes))
    up = q.copy()
    up["position"][0, 2] += 2.0 ** -19                                        # the same vertex 2^-20 above it: separated, and close
    h = tdm.terrain_distance(tm.Terrain(*f), tc.polytopes(), up)[0]
    # (the cube's edge up the y axis runs along the slope at the vertex's height: the terrain edges it crosses are as near)
    assert h["feature"] in (FEATURE_FACE_B, FEATURE_EDGES) and 0.0 < h["distance"] < 2.0 ** -20
    f, q = CASES["cube_on_ridge"]                                             # the ridge pokes 0.05 into the bottom face: rule (ii) alone
    vol = tdm.volume_of(q[0], shapes)
    assert not tdm.vertex_under_ground(surface(f), vol) and tdm.edge_hits_volume(surface(f), vol)
    assert is_overlap(answer("cube_on_ridge"))
    h = answer("cube_over_ridge")                                             # lifted clear
    assert h["feature"] in (FEATURE_FACE_A, FEATURE_EDGES) and h["distance"] == tc.LIFT and list(h["normal"]) == [0.0, 0.0, 1.0]
    assert is_overlap(answer("one_cell_cube_around"))                         # the whole field inside the cube, its vertices beside it


def test_max_distance_at_the_distance_hits_and_one_ulp_below_it_misses():
    h = answer("cube_over_peak_at_reach")
    assert h["body"] == HIT_TERRAIN and h["distance"] == 0.5 and h["feature"] == FEATURE_FACE_A
    assert is_miss(answer("cube_over_peak_below_reach"))


def test_the_one_cell_field_and_queries_that_find_nothing():
    h = answer("one_cell_over_triangle")
    assert h["feature"] == FEATURE_FACE_B and h["index_b"] == 0 and h["distance"] == 0.5
    h = answer("one_cell_over_diagonal")                                      # both triangles tie over the diagonal: the lower one wins
    assert h["feature"] == FEATURE_FACE_B and h["index_b"] == 0 and h["distance"] == 0.5
    h = answer("one_cell_beside_corner")
    assert h["feature"] == FEATURE_EDGES and h["index_b"] == 0 and h["distance"] == math.sqrt(0.5) and list(h["point_b"]) == [-1.0, 2.0, 0.25]
    assert is_overlap(answer("one_cell_under"))
    f, q = CASES["point_over_triangle"]
    for change in ({"max_distance": -1.0}, {"max_distance": np.nan}, {"shape": 1}, {"position": [[np.inf, 0.0, 0.0]]}, {"rotation": [[np.nan, 0.0, 0.0, 0.0]]}):
        bad = q.copy()
        for k, v in change.items():
            bad[k] = v
        assert is_miss(tdm.terrain_distance(tm.Terrain(*f), tc.polytopes(), bad)[0]), change


# ---- random cubes against dense sampling -----------------------------------------------------------------------------------------
STEPS = 40


def random_scene(seed=1, n=300):
    """The draw.  A terrain edge that clips the box by a chord shorter than a step of the sampling grid is OVERLAP through rule
    (ii) with no sample inside the box: the samples cannot see it.  About one draw in three of this recipe holds such a cube
    (seeds 2 and 4 of 1 .. 7 do: sampled distances below a millimetre against a grid step of 36 mm); this one holds none, so
    every case is checked and none is skipped."""
    rng = np.random.default_rng(seed)
    nx, ny, cell = 6, 5, (0.7, 0.9)
    heights = rng.uniform(0.0, 1.2, (ny, nx))
    origin = (0.0, 0.0)
    span = ((nx - 1) * cell[0], (ny - 1) * cell[1])
    centres = np.stack([rng.uniform(-1.0, span[0] + 0.3, n), rng.uniform(-1.0, span[1] + 0.3, n), rng.uniform(0.3, 2.5, n)], axis=1)
    quats = rng.normal(size=(n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    return heights, origin, cell, centres, quats


def surface_samples(heights, origin, cell):
    """Every triangle on a barycentric grid of STEPS steps, and the longest triangle edge."""
    ny, nx = heights.shape
    P = lambda i, j: np.array([origin[0] + i * cell[0], origin[1] + j * cell[1], heights[j, i]])
    bary = np.array([(a, b, STEPS - a - b) for a in range(STEPS + 1) for b in range(STEPS + 1 - a)], dtype=np.float64) / STEPS
    points, longest = [], 0.0
    for j in range(ny - 1):
        for i in range(nx - 1):
            for tri in ((P(i, j), P(i + 1, j), P(i + 1, j + 1)), (P(i, j), P(i + 1, j + 1), P(i, j + 1))):
                points.append(bary @ np.array(tri))
                longest = max(longest, max(float(np.linalg.norm(tri[a] - tri[b])) for a, b in ((0, 1), (1, 2), (2, 0))))
    return np.concatenate(points), longest


def test_random_cubes_agree_with_dense_sampling_of_the_surface():
    heights, origin, cell, centres, quats = random_scene()
    terrain = tm.Terrain(heights, origin, cell)
    cube = rm.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    queries = np.concatenate([tdm.dm.one(tuple(c), rotation=tuple(q), shape=0) for c, q in zip(centres, quats)])
    hits = tdm.terrain_distance(terrain, [cube], queries)
    samples, longest = surface_samples(heights, origin, cell)
    resolution = longest / STEPS            # every point of a triangle is within one grid step's longest edge of a grid point
    separated = overlaps = 0
    for k, h in enumerate(hits):
        pos, rot = tuple(centres[k]), tuple(quats[k])
        inv_pos, inv_rot = tdm.frame_inverse(pos, rot)
        local = np.array(tdm.frame_mul(inv_pos, inv_rot, tdm.cols(samples))).T
        beyond = np.abs(local) - 0.5                                          # the exact point-to-box distance, in the box's frame
        sampled = float(np.sqrt((np.maximum(beyond, 0.0) ** 2).sum(axis=1)).min())
        assert h["body"] == HIT_TERRAIN                                       # max_distance is +inf: the terrain always answers
        if h["feature"] == OVERLAP:
            overlaps += 1
            world = np.array(tdm.frame_mul(pos, rot, tdm.cols(np.asarray(cube["vertices"])))).T
            under = any(p is not None and rm.dot(p[0], tuple(x)) - p[1] < 0.0 for x in world for p in [terrain.plane(tuple(float(c) for c in x))])
            assert under or bool((beyond <= 0.0).all(axis=1).any()), k
        else:
            separated += 1
            d = float(h["distance"])
            assert d <= sampled + 1e-9, (k, d, sampled)
            assert d >= sampled - resolution, (k, d, sampled, resolution)
            gap = np.asarray(h["point_a"]) - np.asarray(h["point_b"])
            assert abs(float(np.linalg.norm(gap)) - d) <= 1e-12 * (1.0 + d)
    print("separated %d, overlaps %d, resolution %.4f" % (separated, overlaps, resolution))
    assert separated + overlaps == len(hits) and separated >= 100 and overlaps >= 30
