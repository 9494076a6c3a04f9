"""The distance model (tests/distance_model.py) on its own: known answers with exactly representable numbers, and on random box and
hull pairs the witness points, the distance between them and the separating-slab certificate that make an answer THE distance."""
import ctypes as C
import math

import numpy as np

import distance_model as dm
import oracle_binding as ob
import raycast_model as rm
from test_sweep_model import random_pairs

IDENT = (1.0, 0.0, 0.0, 0.0)
# Witness points lie on their polytopes, are `distance` apart and the slab between them is empty, all to DELTA * (r_a + r_b +
# distance): the scale the sweep model's test uses.
DELTA = 1e-9


def scene(position, rotation=IDENT, poly=None, volume=None):
    return dm.Scene(np.array([rm.rigid(position, rotation)]), [0], [poly or rm.box()] + ([volume] if volume else []))


def test_two_unit_boxes_three_metres_apart_are_two_metres_apart_through_a_face():
    h = scene((3.0, 0.0, 0.0)).distance(dm.one((0.0, 0.0, 0.0), shape=0))[0]
    assert h["body"] == 0 and h["distance"] == 2.0 and h["feature"] == dm.FEATURE_FACE_B
    assert h["index_a"] == 1 and h["index_b"] == 4                            # the first vertex at x = 1 over the body's -x face
    assert list(h["normal"]) == [-1.0, 0.0, 0.0] and list(h["point_a"]) == [1.0, 0.0, 0.0] and list(h["point_b"]) == [3.0, 0.0, 0.0]
    back = scene((-3.0, 0.0, 0.0)).distance(dm.one((0.0, 0.0, 0.0), shape=0))[0]
    assert back["distance"] == 2.0 and list(back["normal"]) == [1.0, 0.0, 0.0] and back["feature"] in (dm.FEATURE_FACE_A, dm.FEATURE_FACE_B)


def test_boxes_offset_along_the_diagonal_meet_corner_to_corner():
    s = scene((2.0, 2.0, 2.0))
    h = s.distance(dm.one((0.0, 0.0, 0.0), shape=0))[0]
    assert h["body"] == 0 and h["feature"] == dm.FEATURE_EDGES and h["distance"] == math.sqrt(3.0)
    assert list(h["point_a"]) == [1.0, 1.0, 1.0] and list(h["point_b"]) == [2.0, 2.0, 2.0]
    inv = 1.0 / math.sqrt(3.0)
    assert list(h["normal"]) == [-1.0 * inv] * 3
    # max_distance one ulp below the answer misses; equal to it, it hits
    below = s.distance(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=np.nextafter(math.sqrt(3.0), 0.0)))[0]
    assert below["body"] == dm.NO_HIT and below["distance"] == np.inf and below["feature"] == 0
    assert below["index_a"] == dm.NO_HIT and below["index_b"] == dm.NO_HIT
    assert not below["point_a"].any() and not below["point_b"].any() and not below["normal"].any()
    assert s.distance(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=math.sqrt(3.0)))[0]["body"] == 0


def test_crossed_cubes_are_nearest_through_two_edge_interiors():
    cube = rm.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    c, s = math.cos(math.pi / 8.0), math.sin(math.pi / 8.0)
    h = scene((0.0, 3.0, 0.0), (c, s, 0.0, 0.0), cube).distance(dm.one((0.0, 0.0, 0.0), rotation=(c, 0.0, 0.0, s), shape=0))[0]
    assert h["body"] == 0 and h["feature"] == dm.FEATURE_EDGES
    assert abs(h["distance"] - (3.0 - math.sqrt(2.0))) < 1e-14
    assert np.allclose(h["point_a"], [0.0, math.sqrt(0.5), 0.0], atol=1e-15) and np.allclose(h["point_b"], [0.0, 3.0 - math.sqrt(0.5), 0.0], atol=1e-15)
    assert np.allclose(h["normal"], [0.0, -1.0, 0.0], atol=1e-15)
    # both closest points are interior to their edges: neither is a vertex of its cube
    for p, (pos, q) in ((h["point_a"], ((0.0, 0.0, 0.0), (c, 0.0, 0.0, s))), (h["point_b"], ((0.0, 3.0, 0.0), (c, s, 0.0, 0.0)))):
        world = np.array(dm.frame_mul(pos, q, dm.cols(np.asarray(cube["vertices"])))).T
        assert np.abs(world - p).sum(axis=1).min() > 0.4


def test_the_point_volume_above_a_face_beside_an_edge_and_inside():
    s = scene((0.0, 0.0, 0.0))
    above = s.distance(dm.one((0.5, 0.5, 3.0)))[0]
    assert above["feature"] == dm.FEATURE_FACE_B and above["index_a"] == 0 and above["index_b"] == 1 and above["distance"] == 2.0
    assert list(above["point_a"]) == [0.5, 0.5, 3.0] and list(above["point_b"]) == [0.5, 0.5, 1.0] and list(above["normal"]) == [0.0, 0.0, 1.0]
    beside = s.distance(dm.one((2.0, 2.0, 0.5)))[0]
    assert beside["feature"] == dm.FEATURE_EDGES and beside["index_a"] == 0 and beside["distance"] == math.sqrt(2.0)
    assert list(beside["point_b"]) == [1.0, 1.0, 0.5]
    inside = s.distance(dm.one((0.5, 0.5, 0.5)))[0]
    assert inside["body"] == 0 and inside["feature"] == dm.OVERLAP and inside["distance"] == 0.0
    assert inside["index_a"] == dm.NO_HIT and inside["index_b"] == dm.NO_HIT
    assert not inside["point_a"].any() and not inside["point_b"].any() and not inside["normal"].any()
    # the rotation of a point is not used, but must be finite
    assert s.distance(dm.one((0.5, 0.5, 3.0), rotation=(0.0, 0.0, 0.0, 0.0)))[0]["distance"] == 2.0
    assert s.distance(dm.one((0.5, 0.5, 3.0), rotation=(np.nan, 0.0, 0.0, 0.0)))[0]["body"] == dm.NO_HIT


def test_boxes_in_exact_face_touch_are_separated_at_distance_zero():
    h = scene((1.0, 0.0, 0.0)).distance(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=0.0))[0]
    assert h["body"] == 0 and h["distance"] == 0.0 and h["feature"] == dm.FEATURE_FACE_B      # a real feature, not OVERLAP
    # (the first candidate at d2 = 0: the volume's vertex (1, 0, 0) is a corner of the body and lies in its first face, -z, too)
    assert h["index_a"] == 1 and h["index_b"] == 0 and list(h["point_a"]) == list(h["point_b"]) == [1.0, 0.0, 0.0]
    assert not h["normal"].any()
    # a hair into it, the overlap query's verdict
    deep = scene((1.0 - 2.0 ** -20, 0.0, 0.0)).distance(dm.one((0.0, 0.0, 0.0), shape=0))[0]
    assert deep["feature"] == dm.OVERLAP and deep["distance"] == 0.0


def test_queries_that_find_nothing_ties_and_filters():
    s = dm.Scene(np.array([rm.rigid((3.0, 0.0, 0.0)), rm.rigid((5.0, 0.0, 0.0)), rm.rigid((3.0, 0.0, 0.0))]), [0, 0, 0], [rm.box()], groups=[0, 2, 2])
    hit = lambda q, masked=False: s.distance(q, masked)[0]
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0))["body"] == 0                    # equal distances: the smaller index
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, ignore=0))["body"] == 2
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, mask=2), masked=True)["body"] == 2
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, mask=2))["body"] == 0            # without the flag no group is tested
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, mask=1), masked=True)["body"] == dm.NO_HIT
    assert hit(dm.one((0.0, 0.0, 0.0), shape=1))["body"] == dm.NO_HIT
    assert hit(dm.one((0.0, np.inf, 0.0), shape=0))["body"] == dm.NO_HIT
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=-1.0))["body"] == dm.NO_HIT
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=np.nan))["body"] == dm.NO_HIT
    assert hit(dm.one((0.0, 0.0, 0.0), shape=0, max_distance=1.5))["body"] == dm.NO_HIT


def check_pair(L, cache, pa, pb, pos_a, qa, pos_b, qb):
    """Every property of the issue for one pair; returns the feature."""
    s = dm.Scene(np.array([rm.rigid(pos_b, qb)]), [1], [pa, pb])
    h = s.distance(dm.one(pos_a, rotation=qa, shape=0))[0]
    assert h["body"] == 0
    for p in (pa, pb):
        if id(p) not in cache:
            cache[id(p)] = (dm.om.oracle_polytope(p), rm.polytope_planes(p), np.asarray(p["vertices"], dtype=np.float64).reshape(-1, 3))
    m = ob.Manifold()
    L.op_sat(ob.frame(pos_a, qa), ob.frame(pos_b, qb), C.byref(cache[id(pa)][0]), C.byref(cache[id(pb)][0]), C.byref(m))
    assert (h["feature"] != dm.OVERLAP) == bool(m.separated)
    if h["feature"] == dm.OVERLAP:
        assert h["distance"] == 0.0
        return int(h["feature"])
    d = float(h["distance"])
    delta = DELTA * (dm.om.shape_radius(pa) + dm.om.shape_radius(pb) + d)
    # both witness points satisfy every face plane of their polytope
    for point, (pos, q), (_, planes, _) in ((h["point_a"], (pos_a, qa), cache[id(pa)]), (h["point_b"], (pos_b, qb), cache[id(pb)])):
        ip, qi = dm.frame_inverse(tuple(pos), tuple(q))
        local = dm.frame_mul(ip, qi, tuple(point))
        assert (planes[:, :3] @ np.array(local) - planes[:, 3]).max() <= delta
    assert abs(float(np.linalg.norm(h["point_a"] - h["point_b"])) - d) <= delta
    # the certificate: the slab of width `distance` along the normal holds no vertex of either
    aw = np.array(dm.frame_mul(tuple(pos_a), tuple(qa), dm.cols(cache[id(pa)][2]))).T
    bw = np.array(dm.frame_mul(tuple(pos_b), tuple(qb), dm.cols(cache[id(pb)][2]))).T
    assert (aw @ h["normal"]).min() - (bw @ h["normal"]).max() >= d - delta
    # the normal is a unit vector up to the cancellation in point_a - point_b: a few ulps of the points' size over the distance
    size = float(np.abs(h["point_a"]).max() + np.abs(h["point_b"]).max())
    assert d == 0.0 or abs(float(np.linalg.norm(h["normal"])) - 1.0) <= 8.0 * np.finfo(np.float64).eps * size / d + 1e-15
    return int(h["feature"])


def test_random_pairs_have_witnesses_and_a_certificate():
    """600 box and hull pairs in generic position (the sweep model test's generator), every one checked, none skipped; and the
    same pairs once more with the volume moved most of the way towards the body, where some overlap and the others are close."""
    pairs = random_pairs(600, 2024)
    L = ob.load()
    L.op_sat.restype, L.op_sat.argtypes = None, [ob.Frame, ob.Frame, C.POINTER(ob.Polytope), C.POINTER(ob.Polytope), C.POINTER(ob.Manifold)]
    cache, far, near = {}, [], []
    for pa, pb, (pos_a, qa), (pos_b, qb), _ in pairs:
        far.append(check_pair(L, cache, pa, pb, pos_a, qa, pos_b, qb))
        near.append(check_pair(L, cache, pa, pb, pos_b + (pos_a - pos_b) * 0.4, qa, pos_b, qb))
    assert dm.OVERLAP not in far and set(far) == {dm.FEATURE_FACE_A, dm.FEATURE_FACE_B, dm.FEATURE_EDGES}
    assert set(near) == {dm.FEATURE_FACE_A, dm.FEATURE_FACE_B, dm.FEATURE_EDGES, dm.OVERLAP}
