"""Terrain distance queries on the device (include/xpbd.h, "Terrain in the distance queries"): the ring walk, the brute-force pass
over every sample and the independent model (tests/terrain_distance_model.py) agree bit for bit in every field of every hit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_model as dm
import terrain_distance_cases as tc
import terrain_distance_model as tdm
import terrain_model as tm
import terrain_query_model as tq
import test_gpu_overlap as ov
from constraint_solver_amd import capi
from halo_common import pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
BRUTE, MASKED = capi.DISTANCE_BRUTE_FORCE, capi.DISTANCE_MASKED
BOXES, MIXED = capi.SCENE_BOXES_DROP, capi.SCENE_MIXED_DROP
POINT = capi.DISTANCE_POINT
IDENT = [1.0, 0.0, 0.0, 0.0]
INF = np.inf
RECIPE = (tq.recipe_heights(), tq.RECIPE_ORIGIN, tq.RECIPE_CELL)           # 9 x 7, cells of 0.7 x 0.9
PILE_TERRAIN = (tm.bumpy_field(9, 7, 11), (-8.0, -1.5), (1.3, 1.1))         # test_gpu_terrain.py's field under its 96-box pile


def same(a, b):
    return a.dtype.itemsize == b.dtype.itemsize == 96 and len(a) == len(b) and a.tobytes() == b.tobytes()


def first_difference(a, b):
    for k in range(min(len(a), len(b))):
        if a[k:k + 1].tobytes() != b[k:k + 1].tobytes():
            return "record %d: %s != %s" % (k, a[k], b[k])
    return "lengths %d, %d" % (len(a), len(b))


def world(field, polys=None, bodies=None, sid=None):
    w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=True)
    if polys is not None:
        w.set_polytopes(polys)
    if bodies is not None:
        w.upload(bodies, sid)
    if field is not None:
        w.set_terrain(*field)
    return w


def walk_brute_model(w, field, polys, q):
    """The walk, brute force and the model agree in every field of every hit; the model's records."""
    want = tdm.terrain_distance(tm.Terrain(*field), polys, q)
    walk, brute = w.terrain_distance(q), w.terrain_distance(q, BRUTE)
    assert same(walk, brute), first_difference(walk, brute)
    assert same(walk, want), first_difference(walk, want)
    return want


def census(hits):
    """The share of each kind of answer: FACE_A, FACE_B, EDGES, OVERLAP, miss."""
    found = hits["body"] == capi.HIT_TERRAIN
    assert ((hits["body"] == capi.NO_HIT) | found).all()
    n = float(len(hits))
    return {"FACE_A": np.sum(found & (hits["feature"] == capi.FEATURE_FACE_A)) / n, "FACE_B": np.sum(found & (hits["feature"] == capi.FEATURE_FACE_B)) / n,
            "EDGES": np.sum(found & (hits["feature"] == capi.FEATURE_EDGES)) / n, "OVERLAP": np.sum(found & (hits["feature"] == capi.DISTANCE_OVERLAP)) / n,
            "miss": np.sum(~found) / n}


def ground_height(field, x, y):
    """The heights of `field`'s surface under the points (x, y), NaN outside it."""
    terrain = tm.Terrain(*field)
    return np.array([terrain.sample(float(a), float(b))[0] for a, b in zip(x, y)])


def recipe_queries(rng, n, field, n_shapes):
    """n queries in eight families of equal share over `field`: points above, below and beside it; the scene's shapes at random
    poses near the ground with max_distance from 0 to +inf; cubes set down flat over a sample, a face towards it; shapes far
    above with a short reach; and records that can find nothing."""
    heights, origin, cell = field
    ny, nx = heights.shape
    lo = np.array(origin)
    hi = lo + [(nx - 1) * cell[0], (ny - 1) * cell[1]]
    k = n // 8
    quats = lambda m: ov.unit_quaternions(rng, m)
    inside = lambda m: rng.uniform(lo + 0.05, hi - 0.05, (m, 2))
    reaches = lambda m: np.where(np.arange(m) % 4 == 0, INF, np.where(np.arange(m) % 4 == 1, 0.0, rng.uniform(0.05, 1.5, m)))
    parts = []
    xy = inside(k)                                                          # points above the field
    parts.append(capi.distances(np.column_stack([xy, ground_height(field, xy[:, 0], xy[:, 1]) + rng.uniform(0.01, 1.5, k)]), [IDENT], POINT,
                                max_distance=np.where(np.arange(k) % 3 == 0, INF, 2.0)))
    xy = inside(k)                                                          # points below its surface
    parts.append(capi.distances(np.column_stack([xy, ground_height(field, xy[:, 0], xy[:, 1]) - rng.uniform(0.01, 1.0, k)]), [IDENT], POINT))
    side = rng.integers(0, 4, k)                                            # points beside it, above and below its border's height
    xy = inside(k)
    off = rng.uniform(0.05, 1.5, k)
    xy[:, 0] = np.where(side == 0, lo[0] - off, np.where(side == 1, hi[0] + off, xy[:, 0]))
    xy[:, 1] = np.where(side == 2, lo[1] - off, np.where(side == 3, hi[1] + off, xy[:, 1]))
    parts.append(capi.distances(np.column_stack([xy, rng.uniform(-1.5, 1.5, k)]), [IDENT], POINT, max_distance=np.where(np.arange(k) % 4 == 0, 0.3, INF)))
    for _ in range(2):                                                      # shapes at random poses near the ground, twice
        xy = rng.uniform(lo - 0.8, hi + 0.8, (k, 2))
        z = np.nan_to_num(ground_height(field, np.clip(xy[:, 0], lo[0], hi[0] - 1e-9), np.clip(xy[:, 1], lo[1], hi[1] - 1e-9))) + rng.uniform(0.2, 1.6, k)
        parts.append(capi.distances(np.column_stack([xy, z]), quats(k), rng.integers(0, n_shapes, k), max_distance=reaches(k)))
    # the unit cube (shape 0) or the tetrahedron (shape 1, when there is one) set down flat over a peak -- a sample above its
    # eight neighbours -- turned about z alone, the middle of its bottom face a little above the peak: the ground nearest to a
    # flat face is the highest point under it
    peaks = [(a, b) for b in range(1, ny - 1) for a in range(1, nx - 1) if heights[b, a] > np.delete(heights[b - 1:b + 2, a - 1:a + 2].ravel(), 4).max()]
    assert peaks, "the field needs a peak"
    i, j = np.array(peaks)[rng.integers(0, len(peaks), k)].T
    yaw = rng.uniform(0.0, 2.0 * np.pi, k)
    rot = np.column_stack([np.cos(0.5 * yaw), np.zeros(k), np.zeros(k), np.sin(0.5 * yaw)])
    shape = np.arange(k) % min(n_shapes, 2)
    mid = np.where(shape == 0, 0.5, 1.0 / 6.0)                              # of the bottom face, in the shape's own x and y
    flat = capi.distances(np.column_stack([lo[0] + i * cell[0], lo[1] + j * cell[1], heights[j, i] + rng.uniform(0.02, 0.3, k)]), rot, shape,
                          max_distance=np.where(np.arange(k) % 5 == 0, 0.5, INF))
    flat["position"][:, :2] -= np.column_stack([(np.cos(yaw) - np.sin(yaw)) * mid, (np.sin(yaw) + np.cos(yaw)) * mid])
    parts.append(flat)
    xy = inside(k)                                                          # far above, a short reach: misses
    parts.append(capi.distances(np.column_stack([xy, rng.uniform(3.0, 6.0, k)]), quats(k), np.where(np.arange(k) % 2 == 0, POINT, 0),
                                max_distance=rng.uniform(0.0, 1.0, k)))
    rest = n - sum(len(p) for p in parts)                                   # records that can find nothing
    bad = capi.distances(np.column_stack([inside(rest), np.ones(rest)]), quats(rest), np.where(np.arange(rest) % 2 == 0, POINT, 0))
    for r in range(rest):
        case = r % 4
        if case == 0:
            bad["position" if r % 8 < 4 else "rotation"][r, r % 3] = (np.nan, np.inf, -np.inf)[(r // 4) % 3]
        elif case == 1:
            bad["shape"][r] = n_shapes + (r // 4) % 2 * 1000
        elif case == 2:
            bad["max_distance"][r] = -1.0e-300 if (r // 4) % 2 else -2.0
        else:
            bad["max_distance"][r] = np.nan
    parts.append(bad)
    return np.concatenate(parts)


# ---- 1. crafted queries at binary spacing ------------------------------------------------------------------------------------------
def test_crafted_queries_equal_the_model_bit_for_bit():
    polys = tc.polytopes()
    for field, names, q in tc.by_field():
        with world(field, polys) as w:
            want = walk_brute_model(w, field, polys, q)
            assert len(want) == len(names)
            for k in range(len(q)):                                         # one at a time too: a group on its own in its block
                assert same(w.terrain_distance(q[k:k + 1]), want[k:k + 1]), names[k]


# ---- 2. random queries in families ------------------------------------------------------------------------------------------------
def test_random_queries_equal_the_model_and_every_kind_of_answer_occurs():
    polys = capi.scene_polytopes(MIXED)
    q = recipe_queries(np.random.default_rng(2024), 512, RECIPE, len(polys))
    assert len(q) == 512
    with world(RECIPE, polys) as w:
        want = walk_brute_model(w, RECIPE, polys, q)
        shares = census(want)
        print(shares)
        assert all(share >= 0.05 for share in shares.values()), shares
        for n in (1, 9, 67):                                                # partial groups and blocks
            assert same(w.terrain_distance(q[100:100 + n]), want[100:100 + n])
        masked = q.copy()                                                   # the flags of a body call are accepted; ignore_body and mask are not read
        masked["ignore_body"], masked["mask"] = capi.HIT_TERRAIN, 0
        assert same(w.terrain_distance(masked, MASKED), want) and same(w.terrain_distance(masked, MASKED | BRUTE), want)
    with world(RECIPE) as w:                                                # no polytopes: only the points find anything
        points = q["shape"] == POINT
        bare = w.terrain_distance(q)
        assert same(bare[points], want[points]) and (bare["body"][~points] == capi.NO_HIT).all() and np.isinf(bare["distance"][~points]).all()
        assert same(w.terrain_distance(q, BRUTE), bare)


# ---- 3. many rings, many blocks --------------------------------------------------------------------------------------------------
def test_long_walks_on_a_large_field_equal_brute_force():
    heights = tq.recipe_heights(65, 65)
    field = (heights, (-8.0, -8.0), (0.25, 0.25))
    polys = capi.scene_polytopes(MIXED)
    rng = np.random.default_rng(65)
    n = 1025
    pos = np.column_stack([rng.uniform(-9.0, 9.0, n), rng.uniform(-9.0, 9.0, n), rng.uniform(0.7, 6.0, n)])
    pos[::16] += [20.0, 0.0, 0.0]                                           # far beside the field
    q = capi.distances(pos, ov.unit_quaternions(rng, n), np.where(np.arange(n) % 3 == 0, POINT, np.arange(n) % 3))
    with world(field, polys) as w:
        walk, brute = w.terrain_distance(q), w.terrain_distance(q, BRUTE)
        assert same(walk, brute), first_difference(walk, brute)
        assert (walk["body"] == capi.HIT_TERRAIN).all() and (walk["distance"] > 1.0).sum() > 300       # regions wider than a group's lanes
        assert same(w.terrain_distance(q[:1024]), walk[:1024])
        some = np.arange(0, n, 41)                                          # 25 of them against the model
        assert same(walk[some], tdm.terrain_distance(tm.Terrain(*field), polys, q[some]))


def test_a_polytope_of_32_vertices():
    from test_gpu_distance import random_simple_polytope
    polys = [random_simple_polytope(5), capi.polytope(capi.SHAPE_CUBE)]
    assert len(polys[0]["vertices"]) == 32
    rng = np.random.default_rng(32)
    n = 96
    xy = rng.uniform([-3.5, -2.7], [2.9, 3.5], (n, 2))
    q = capi.distances(np.column_stack([xy, rng.uniform(0.2, 2.2, n)]), ov.unit_quaternions(rng, n), 0, max_distance=np.where(np.arange(n) % 3 == 0, 0.5, INF))
    with world(RECIPE, polys) as w:
        want = walk_brute_model(w, RECIPE, polys, q)
        shares = census(want)
        assert shares["OVERLAP"] > 0.1 and shares["FACE_B"] + shares["FACE_A"] + shares["EDGES"] > 0.3, shares


# ---- 4. consistency with the overlap query and with the bodies' distance query -----------------------------------------------------
@pytest.fixture(scope="module")
def settled_pile():
    """The 96-box pile of test_gpu_terrain.py settled on its 9 x 7 field: (state, shape ids)."""
    bodies, sid = pile(capi, BOXES, 96, 3, 4.0, 3.0)
    with world(PILE_TERRAIN, capi.scene_polytopes(BOXES), bodies, sid) as w:
        w.set_max_depenetration_speed(3.0)
        for _ in range(40):
            w.step(DT, 6)
        state = w.download()
    assert not np.isnan(state).any()
    return state, sid


def test_where_the_overlap_query_lists_the_terrain_this_call_says_overlap(settled_pile):
    state, sid = settled_pile
    polys = capi.scene_polytopes(BOXES)
    rng = np.random.default_rng(51)
    k = 256
    pos = np.stack([rng.uniform(-9.5, 6.0, k), rng.uniform(-2.5, 6.5, k), rng.uniform(-0.8, 1.5, k)], axis=1)
    quats = ov.unit_quaternions(rng, k)
    with world(PILE_TERRAIN, polys, state, sid) as w:
        offsets, hits = w.overlap(capi.overlap_queries(pos, quats, 0), capi.QUERY_TERRAIN)
        listed = np.array([(hits["body"][a:b] == capi.HIT_TERRAIN).any() for a, b in zip(offsets[:-1], offsets[1:])])
        got = w.terrain_distance(capi.distances(pos, quats, 0))
        overlap = (got["body"] == capi.HIT_TERRAIN) & (got["feature"] == capi.DISTANCE_OVERLAP)
        assert listed.sum() > 40 and (~listed).sum() > 40
        assert overlap[listed].all()                                        # rule (i) is the overlap query's rule
        assert (got["distance"][~overlap] > 0.0).sum() > 40                 # (rule (ii) may add some: a ridge between the vertices)


def test_the_merge_of_the_two_calls_equals_the_merge_of_the_two_models(settled_pile):
    state, sid = settled_pile
    polys = capi.scene_polytopes(BOXES)
    rng = np.random.default_rng(96)
    k = 192
    pos = np.stack([rng.uniform(-9.0, 5.0, k), rng.uniform(-2.0, 6.0, k), rng.uniform(0.3, 3.0, k)], axis=1)
    q = capi.distances(pos, ov.unit_quaternions(rng, k), np.where(np.arange(k) % 2 == 0, POINT, 0), max_distance=np.where(np.arange(k) % 3 == 0, 1.0, INF))
    want = tdm.merge(dm.Scene(state, sid, polys).distance(q), tdm.terrain_distance(tm.Terrain(*PILE_TERRAIN), polys, q))
    with world(PILE_TERRAIN, polys, state, sid) as w:
        bodies, ground = w.distance(q), w.terrain_distance(q)
        got = np.where(ground["distance"] < bodies["distance"], ground, bodies)                         # a body wins a tie
        assert same(got, want), first_difference(got, want)
        assert (got["body"] == capi.HIT_TERRAIN).sum() > 30 and (got["body"] < 96).sum() > 30 and (got["body"] == capi.NO_HIT).sum() > 5


# ---- 5. errors, the terrain's lifetime, no side effects ---------------------------------------------------------------------------------
def test_the_errors_leave_the_outputs_untouched_and_name_the_call():
    L = capi.hip_lib()
    polys = capi.scene_polytopes(BOXES)
    q = capi.distances(np.zeros((12, 3)) + [0.0, 0.0, 2.0])

    def call(fn, h, queries, n, flags, give_hits=True):
        hits = np.zeros(14, dtype=capi.DISTANCE_HIT_DTYPE)
        hits["body"] = 0xCDCDCDCD
        rc = fn(h, queries.ctypes.data if queries is not None else None, n, flags, hits.ctypes.data if give_hits else None)
        return rc, L.xpbd_last_error(), bool((hits["body"] == 0xCDCDCDCD).all() and not hits["distance"].any())

    host, dev = L.xpbd_world_terrain_distance, L.xpbd_world_terrain_distance_device
    with world(None, polys) as w:                                           # no terrain
        for fn, name in ((host, b"xpbd_world_terrain_distance"), (dev, b"xpbd_world_terrain_distance_device")):
            rc, message, untouched = call(fn, w._h, q, 12, 0)
            assert rc == capi.E_INVALID and b"xpbd_world_set_terrain" in message and name in message and untouched
        w.set_terrain(*RECIPE)
        for fn, name in ((host, b"xpbd_world_terrain_distance"), (dev, b"xpbd_world_terrain_distance_device")):   # (checked before any pointer is touched)
            for flags in (4, capi.QUERY_TERRAIN, capi.QUERY_TERRAIN | BRUTE, 0x80000000):
                rc, message, untouched = call(fn, w._h, q, 12, flags)
                assert rc == capi.E_INVALID and b"unknown flags" in message and name in message and untouched
            rc, message, untouched = call(fn, w._h, None, 12, 0)
            assert rc == capi.E_INVALID and b"NULL" in message and name in message and untouched
            rc, message, untouched = call(fn, w._h, q, 12, 0, give_hits=False)
            assert rc == capi.E_INVALID and b"NULL" in message and name in message
            assert fn(w._h, None, 0, 0, None) == capi.OK                    # n_queries == 0
        reserved = q.copy()
        reserved["reserved"][5] = 1
        rc, message, untouched = call(host, w._h, reserved, 12, 0)
        assert rc == capi.E_INVALID and b"query 5" in message and b"xpbd_world_terrain_distance" in message and untouched
        assert call(host, w._h, q, 12, BRUTE | MASKED)[0] == capi.OK        # every known flag; neither bodies nor a body call needed
        assert (w.terrain_distance(q)["body"] == capi.HIT_TERRAIN).all()
        w.set_terrain(None)                                                 # back to the plane: no terrain again
        rc, message, untouched = call(host, w._h, q, 12, 0)
        assert rc == capi.E_INVALID and b"xpbd_world_set_terrain" in message and untouched


def test_a_second_set_terrain_is_answered_from_the_new_heights():
    q = capi.distances([[-0.3, 0.4, 3.0], [1.1, -0.9, 2.5], [-2.0, 2.0, 4.0]])
    other = (RECIPE[0] + 1.0, RECIPE[1], RECIPE[2])
    small = (np.full((2, 2), -1.0), (-4.0, -4.0), (8.0, 8.0))               # fewer samples than before: the old block is gone
    with world(RECIPE) as w:
        first = walk_brute_model(w, RECIPE, [], q)
        for field in (other, small, RECIPE):
            w.set_terrain(*field)
            got = walk_brute_model(w, field, [], q)
            if field is other:
                nearer = first["distance"] - got["distance"]               # the surface came up by 1: nearer, by at most 1
                assert (nearer > 0.5).all() and (nearer <= 1.0 + 1e-12).all() and not same(got, first)
        assert same(got, first)


def test_stepping_after_the_queries_gives_the_bits_of_stepping_without_them():
    bodies, sid = pile(capi, BOXES, 96, 3, 4.0, 3.0)
    polys = capi.scene_polytopes(BOXES)
    spots = bodies[:64, 31:34] * [1.0, 1.0, 0.1] + [0.0, 0.0, 0.5]
    spots[::2] -= [5.0, 0.0, 0.4]                                           # every other one beside the pile, over the field
    q = capi.distances(spots, [IDENT], np.where(np.arange(64) % 2 == 0, POINT, 0))
    results = []
    for ask in (False, True):
        with world(PILE_TERRAIN, polys, bodies, sid) as w:
            w.set_contact_report(True)
            for _ in range(8):
                w.step(DT, 6)
                if ask:
                    found = w.terrain_distance(q)
                    assert (found["body"] == capi.HIT_TERRAIN).all() and same(w.terrain_distance(q, BRUTE), found)
            results.append((w.download(), w.contacts(), w.contact_masks(6), np.array(w.contact_stats(), dtype=np.uint64),
                            np.array(w.contact_report_counts(), dtype=np.uint64)))
    for a, b in zip(*results):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert results[0][2].any() and not np.isnan(results[0][0]).any()


# ---- 6. the device variant ----------------------------------------------------------------------------------------------------------
def test_the_device_variant_equals_the_host_variant():
    """In a fresh child process that imports torch first (the library then binds to the HIP runtime torch carries)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "terrain_distance_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res and all(res.values()), res
    assert set(res) >= {"walk", "brute", "masked", "guard", "terrain_seen", "no_terrain_is_invalid"}
