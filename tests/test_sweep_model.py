"""The sweep model (tests/sweep_model.py) on its own: known answers with exactly representable numbers, and a cross-check of
its times of impact against the oracle's SAT -- separated just before the impact, not separated just after it."""
import ctypes as C
import math

import numpy as np

import hull_util as hu
import oracle_binding as ob
import raycast_model as rm
import sweep_model as sm

IDENT = (1.0, 0.0, 0.0, 0.0)
SWEEP = np.dtype([("position", "<f8", (3,)), ("rotation", "<f8", (4,)), ("direction", "<f8", (3,)), ("max_distance", "<f8"),
                  ("shape", "<u4"), ("ignore_body", "<u4"), ("mask", "<u4"), ("reserved", "<u4")])
# The oracle's verdicts bracket the model's t at DELTA * (r_a + r_b).  1e-9 is where the search for it starts, and all 600 pairs
# pass there (they still do at 1e-13), so no larger power of ten was needed.
DELTA = 1e-9


def one(position, direction, max_distance=np.inf, rotation=IDENT, shape=0, ignore=sm.NO_HIT):
    q = np.zeros(1, dtype=SWEEP)
    q["position"], q["rotation"], q["direction"], q["max_distance"], q["shape"] = position, rotation, direction, max_distance, shape
    q["ignore_body"], q["mask"] = ignore, 0xFFFFFFFF
    return q


def unit_box_scene(position, rotation=IDENT, poly=None):
    return sm.Scene(np.array([rm.rigid(position, rotation)]), [0], [poly or rm.box()])


def test_a_box_swept_at_a_box_hits_its_face_at_two():
    scene = unit_box_scene((3.0, 0.0, 0.0))
    h = scene.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))[0]
    assert h["body"] == 0 and h["distance"] == 2.0 and h["feature"] in (sm.FEATURE_FACE_A, sm.FEATURE_FACE_B)
    assert h["feature"] == sm.FEATURE_FACE_A and h["face"] == 5                   # the first of the constraints that tie: the volume's +x face
    assert list(h["normal"]) == [-1.0, 0.0, 0.0] and list(h["position"]) == [2.0, 0.0, 0.0] and h["reserved"] == 0


def test_the_same_sweep_cut_short_misses():
    scene = unit_box_scene((3.0, 0.0, 0.0))
    h = scene.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.5))[0]
    assert h["body"] == sm.NO_HIT and h["feature"] == 0 and h["face"] == sm.NO_HIT and h["distance"] == np.inf
    assert not h["position"].any() and not h["normal"].any()
    assert scene.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 2.0))[0]["distance"] == 2.0      # max_distance itself still hits


def test_a_volume_that_starts_overlapping_reports_the_initial_overlap():
    scene = unit_box_scene((0.5, 0.0, 0.0))
    h = scene.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))[0]
    assert h["body"] == 0 and h["feature"] == sm.SWEEP_INITIAL and h["face"] == sm.NO_HIT and h["distance"] == 0.0
    assert not h["normal"].any() and not h["position"].any()


def test_a_box_sliding_along_another_in_exact_touch_misses():
    scene = unit_box_scene((0.0, 1.0, 0.0))
    assert scene.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))[0]["body"] == sm.NO_HIT
    assert scene.sweep(one((-5.0, 0.0, 0.0), (1.0, 0.0, 0.0)))[0]["body"] == sm.NO_HIT
    # ... and a hair into it, it hits
    assert scene.sweep(one((-5.0, 2.0 ** -20, 0.0), (1.0, 0.0, 0.0)))[0]["distance"] == 4.0


def test_a_sweep_pointing_away_misses():
    scene = unit_box_scene((3.0, 0.0, 0.0))
    assert scene.sweep(one((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0)))[0]["body"] == sm.NO_HIT


def test_crossed_edges_enter_through_the_edge_feature():
    """A cube turned 45 degrees about z moves along +y at a cube turned 45 degrees about x: its leading edge (along z) meets the
    other's leading edge (along x) at a point."""
    cube = rm.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    c, s = math.cos(math.pi / 8.0), math.sin(math.pi / 8.0)
    scene = unit_box_scene((0.0, 3.0, 0.0), (c, s, 0.0, 0.0), cube)
    h = scene.sweep(one((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), rotation=(c, 0.0, 0.0, s)))[0]
    assert h["body"] == 0 and h["feature"] == sm.FEATURE_EDGES and h["face"] == sm.NO_HIT
    assert abs(h["distance"] - (3.0 - math.sqrt(2.0))) < 1e-14
    assert np.allclose(h["normal"], [0.0, -1.0, 0.0], atol=1e-15) and np.allclose(h["position"], [0.0, h["distance"], 0.0], atol=0.0)


def test_a_direction_twice_as_long_halves_t():
    scene = unit_box_scene((3.0, 0.0, 0.0))
    h = scene.sweep(one((0.0, 0.0, 0.0), (2.0, 0.0, 0.0)))[0]
    assert h["distance"] == 1.0 and list(h["position"]) == [2.0, 0.0, 0.0] and list(h["normal"]) == [-1.0, 0.0, 0.0]


def test_sweeps_that_cannot_hit_anything_and_ignored_bodies():
    scene = sm.Scene(np.array([rm.rigid((3.0, 0.0, 0.0)), rm.rigid((5.0, 0.0, 0.0))]), [0, 0], [rm.box()])
    hit = lambda q: scene.sweep(q)[0]
    assert hit(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))["body"] == 0
    assert hit(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), ignore=0))["distance"] == 4.0
    assert hit(one((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))["body"] == sm.NO_HIT
    assert hit(one((0.0, np.nan, 0.0), (1.0, 0.0, 0.0)))["body"] == sm.NO_HIT
    assert hit(one((0.0, 0.0, 0.0), (1.0, np.inf, 0.0)))["body"] == sm.NO_HIT
    assert hit(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), -1.0))["body"] == sm.NO_HIT
    assert hit(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.nan))["body"] == sm.NO_HIT
    assert hit(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), shape=1))["body"] == sm.NO_HIT
    # equal t: the smaller index
    twins = sm.Scene(np.array([rm.rigid((3.0, 0.0, 0.0)), rm.rigid((3.0, 0.0, 0.0))]), [0, 0], [rm.box()])
    assert twins.sweep(one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))[0]["body"] == 0
    masked = sm.Scene(np.array([rm.rigid((3.0, 0.0, 0.0)), rm.rigid((5.0, 0.0, 0.0))]), [0, 0], [rm.box()], groups=[0, 2])
    q = one((0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    q["mask"] = 2
    assert masked.sweep(q)[0]["body"] == 0 and masked.sweep(q, masked=True)[0]["body"] == 1


def random_pairs(n, seed):
    """n (polytope dict A, polytope dict B, frame of A, frame of B, unit direction) in generic position: A starts clear of B and
    moves at it, its centroid aimed at a point near B's."""
    rng = np.random.default_rng(seed)
    hulls = [hu.as_capi(*hu.random_hull(100 + k, 6 + 2 * k, 0.4 + 0.05 * k)) for k in range(6)]
    cube = rm.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    out = []
    for k in range(n):
        pa = cube if k % 3 == 0 else hulls[int(rng.integers(0, len(hulls)))]
        pb = cube if k % 3 != 2 else hulls[int(rng.integers(0, len(hulls)))]
        qa, qb = rng.normal(size=4), rng.normal(size=4)
        qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
        away = rng.normal(size=3)
        away /= np.linalg.norm(away)
        reach = sm.shape_radius(pa) + sm.shape_radius(pb)
        pos_b = rng.uniform(-2.0, 2.0, 3)
        pos_a = pos_b + away * reach * rng.uniform(1.5, 3.0)
        aim = pos_b + rng.normal(size=3) * 0.02 - pos_a            # (the centroids sit at the frames' origins up to the hulls' offsets)
        out.append((pa, pb, (pos_a, qa), (pos_b, qb), aim / np.linalg.norm(aim)))
    return out


def test_the_oracle_brackets_every_time_of_impact():
    """op_sat says separated at t - delta and not separated at t + delta, delta = DELTA * (r_a + r_b), for every one of 600 box
    and hull pairs; none is skipped (the seed is one for which every pair hits at t > 0, which is asserted).  A DELTA above 1e-6
    would mean the model is wrong, not that the tolerance is small."""
    pairs = random_pairs(600, 2024)
    L = ob.load()
    L.op_sat.restype, L.op_sat.argtypes = None, [ob.Frame, ob.Frame, C.POINTER(ob.Polytope), C.POINTER(ob.Polytope), C.POINTER(ob.Manifold)]
    cache = {}
    features = set()
    for pa, pb, (pos_a, qa), (pos_b, qb), d in pairs:
        scene = sm.Scene(np.array([rm.rigid(pos_b, qb)]), [1], [pa, pb])
        h = scene.sweep(one(pos_a, d, rotation=qa, shape=0))[0]
        assert h["body"] == 0 and h["distance"] > 0.0 and h["feature"] != sm.SWEEP_INITIAL
        features.add(int(h["feature"]))
        for p in (pa, pb):
            if id(p) not in cache:
                cache[id(p)] = sm.oracle_polytope(p)
        reach = sm.shape_radius(pa) + sm.shape_radius(pb)

        def separated(t):
            m = ob.Manifold()
            L.op_sat(ob.frame(pos_a + d * t, qa), ob.frame(pos_b, qb), C.byref(cache[id(pa)]), C.byref(cache[id(pb)]), C.byref(m))
            return bool(m.separated)

        delta = DELTA * reach
        assert separated(h["distance"] - delta) and not separated(h["distance"] + delta)
        # the normal points out of the body towards the volume: against the motion
        assert float(np.dot(h["normal"], d)) < 0.0 and abs(np.linalg.norm(h["normal"]) - 1.0) < 1e-12
    assert features == {sm.FEATURE_FACE_A, sm.FEATURE_FACE_B, sm.FEATURE_EDGES}
