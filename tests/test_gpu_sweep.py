"""Sweep queries on the device (include/xpbd.h, "Sweep queries"): the grid path, the brute-force path and the independent model
(tests/sweep_model.py) agree bit for bit in every field of every hit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_model as rm
import sweep_model as sm
import test_gpu_overlap as ov
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
BRUTE, MASKED = capi.SWEEP_BRUTE_FORCE, capi.SWEEP_MASKED
KIND = capi.SCENE_MIXED_DROP
IDENT = [1.0, 0.0, 0.0, 0.0]
FEATURES = {capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES, capi.SWEEP_INITIAL}


def same_hits(a, b):
    return a.dtype.itemsize == b.dtype.itemsize == 72 and ov.same_bits(a.view(np.uint8), b.view(np.uint8))


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sweep_families(rng, state, sid, polys, n, shapes=None):
    """n sweeps, eight families of equal share, around the bodies of `state`; volumes of the shapes listed (default: all)."""
    k = n // 8
    frames = ov.frames_of(state)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0) - 0.5, centre.max(axis=0) + 0.5
    span = float(np.linalg.norm(hi - lo))
    pool = np.arange(len(polys)) if shapes is None else np.asarray(shapes)
    pick_shapes = lambda m: pool[rng.integers(0, len(pool), m)]
    quats = lambda m: ov.unit_quaternions(rng, m)
    radius = np.array([sm.shape_radius(polys[int(s)]) for s in sid])
    parts = []
    # short sweeps inside the pile's box, directions of any length
    d = unit(rng.normal(size=(k, 3))) * rng.uniform(0.2, 3.0, (k, 1))
    parts.append(capi.sweeps(rng.uniform(lo, hi, (k, 3)), quats(k), d, pick_shapes(k), max_distance=rng.uniform(0.05, 1.5, k)))
    # across the whole pile: from outside its box through a point inside it, no limit
    away = unit(rng.normal(size=(k, 3))) * (0.5 * span + 3.0)
    through = rng.uniform(lo, hi, (k, 3))
    start = 0.5 * (lo + hi) + away
    parts.append(capi.sweeps(start, quats(k), unit(through - start) * rng.uniform(0.5, 2.0, (k, 1)), pick_shapes(k)))
    # axis-aligned directions: two components are zero, or one
    axes = np.zeros((k, 3))
    axes[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0, 2.0, -0.5], k)
    some = np.arange(k) % 3 == 0
    axes[some, rng.integers(0, 3, int(some.sum()))] += 1.0
    axes[(axes == 0.0).all(axis=1)] = [0.0, 0.0, -1.0]
    start = rng.uniform(lo, hi, (k, 3))
    start[::2] -= axes[::2] * span                                   # half of them start outside and run through the pile
    parts.append(capi.sweeps(start, quats(k), axes, pick_shapes(k), max_distance=np.where(np.arange(k) % 4 == 1, 0.75, np.inf)))
    # sphere centres on cell faces: axis-aligned volumes whose centroid sits on multiples of the cell edge
    edge = ov.cell_edge(polys, sid)
    sh = pick_shapes(k)
    centroid = np.array([polys[int(s)]["centroid"] for s in sh])
    on_face = np.round(rng.uniform(lo, hi, (k, 3)) / edge) * edge - centroid
    d = unit(rng.normal(size=(k, 3)))
    d[::2] = axes[::2]
    parts.append(capi.sweeps(on_face, [IDENT], d, sh, max_distance=rng.uniform(0.5, 4.0, k)))
    # starts inside a body: its exact pose and shape, with and without ignoring it
    pick = rng.integers(0, len(state), k)
    ignore = np.where(np.arange(k) % 2 == 0, pick, capi.NO_HIT)
    parts.append(capi.sweeps(frames[pick, :3], frames[pick, 3:], unit(rng.normal(size=(k, 3))), sid[pick], max_distance=rng.uniform(0.1, 2.0, k),
                             ignore=ignore))
    # max_distance 0 (an initial overlap or nothing) and +inf, from poses a fraction of a radius off a body
    pick = rng.integers(0, len(state), k)
    shift = rng.normal(size=(k, 3)) * (0.6 * radius[pick])[:, None]
    parts.append(capi.sweeps(frames[pick, :3] + shift, quats(k), unit(rng.normal(size=(k, 3))), pick_shapes(k),
                             max_distance=np.where(np.arange(k) % 2 == 0, 0.0, np.inf), ignore=np.where(np.arange(k) % 4 < 2, pick, capi.NO_HIT)))
    # grazing: a unit cube (shape 0, spanning [0, 1]^3) slides along x over the highest vertex of a body, its bottom face half a
    # millimetre below the vertex (it hits) or above it (it passes that body)
    pick = rng.integers(0, len(state), k)
    graze = capi.sweeps(np.zeros((k, 3)), [IDENT], [[1.0, 0.0, 0.0]], 0, max_distance=6.0)
    for j in range(k):
        i = int(pick[j])
        v = np.asarray(polys[int(sid[i])]["vertices"], dtype=np.float64)
        world = np.array(rm.rotate(tuple(frames[i, 3:]), tuple(v.T))).T + frames[i, :3]
        top = world[np.argmax(world[:, 2])]
        graze["position"][j] = top - [3.5, 0.5, 5.0e-4 if j % 2 == 0 else -5.0e-4]
    parts.append(graze)
    # records that can hit nothing: zero direction, frame or direction not finite, shape outside the table, max_distance < 0 or NaN
    rest = n - sum(len(p) for p in parts)
    bad = capi.sweeps(frames[rng.integers(0, len(state), rest), :3], quats(rest), unit(rng.normal(size=(rest, 3))), pick_shapes(rest))
    for j in range(rest):
        case = j % 6
        if case == 0:
            bad["direction"][j] = [0.0, -0.0, 0.0]
        elif case == 1:
            bad["position" if j % 4 < 2 else "rotation"][j, j % 3] = (np.nan, np.inf, -np.inf)[(j // 6) % 3]
        elif case == 2:
            bad["direction"][j, j % 3] = (np.nan, np.inf, -np.inf)[(j // 6) % 3]
        elif case == 3:
            bad["shape"][j] = len(polys) + (j // 6) % 2 * 1000
        elif case == 4:
            bad["max_distance"][j] = -1.0e-300 if (j // 6) % 2 else -2.0
        else:
            bad["max_distance"][j] = np.nan
    parts.append(bad)
    return np.concatenate(parts), rest


def check_three_ways(w, scene, q, flags=0):
    want = scene.sweep(q, masked=bool(flags & MASKED))
    grid, brute = w.sweep(q, flags), w.sweep(q, flags | BRUTE)
    assert same_hits(grid, brute)
    assert same_hits(grid, want)
    return want


def world_of(bodies, sid, polys, mode=capi.MODE_CONTACTS):
    w = capi.World(mode=mode)
    w.set_polytopes(polys)
    w.upload(bodies, sid)
    return w


@pytest.mark.parametrize("mode", [capi.MODE_CONTACTS, capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
def test_grid_brute_force_and_model_agree_on_a_mixed_pile(mode):
    bodies, sid = ov.pile()
    polys = capi.scene_polytopes(KIND)
    with ov.stepped(bodies, sid, polys, 1, 10, mode=mode) as w:
        state = w.download()
        q, bad = sweep_families(np.random.default_rng(140 + mode), state, sid, polys, 512)
        hits = check_three_ways(w, sm.Scene(state, sid, polys), q)
    k = len(q) // 8
    found = hits["body"] != capi.NO_HIT
    assert set(hits["feature"][found]) == FEATURES
    assert not found[-bad:].any() and np.mean(found) > 0.5 and np.sum(~found[:-bad]) >= 16
    miss = hits[~found]
    assert (miss["face"] == capi.NO_HIT).all() and np.isinf(miss["distance"]).all() and not miss["feature"].any()
    assert not miss["position"].any() and not miss["normal"].any() and not hits["reserved"].any()
    assert np.mean(found[k:2 * k]) > 0.9                            # sweeps through the pile hit something
    inside = hits[4 * k + 1:5 * k:2]                                # the exact pose of a body, nobody ignored
    assert (inside["feature"] == capi.SWEEP_INITIAL).all() and not inside["distance"].any()
    graze = hits[6 * k:7 * k]
    assert (graze["body"] != capi.NO_HIT).mean() > 0.5
    moving = hits[found & (hits["feature"] != capi.SWEEP_INITIAL)]
    assert (np.einsum("ij,ij->i", moving["normal"], q["direction"][found & (hits["feature"] != capi.SWEEP_INITIAL)]) < 0.0).all()


def test_wide_groups_unstaged_edge_directions_and_large_volumes():
    """Shapes above 16 vertices take the 64-lane groups; 18 vertices have 48 edge directions, more than the 32 that are staged; a
    cube of 2.5 m is larger than a cell and walks boxes of many cells, one of 12 m is beyond the walk and looks at every body."""
    import hull_util as hu
    raw = [hu.random_hull(7, 18, 0.6), hu.random_hull(8, 17, 0.5), hu.random_hull(9, 10, 0.4)]
    polys = [hu.as_capi(*h) for h in raw] + [capi.polytope(capi.SHAPE_CUBE, 2.5), capi.polytope(capi.SHAPE_CUBE, 12.0)]
    assert len(sm.edge_directions(polys[0])) > 32 and max(len(p["vertices"]) for p in polys) == 18
    n = 512
    rng = np.random.default_rng(151)
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, 5, n)
    bodies[:, 31:34] = rng.uniform(0.0, 8.0, (n, 3))
    bodies[:, 34:38] = ov.unit_quaternions(rng, n)
    bodies[:, 28:31] = 0.0                                          # the hulls are centred: com = 0
    sid = (np.arange(n) % 3).astype(np.uint32)
    assert 2.5 > ov.cell_edge(polys, sid) and sm.shape_radius(polys[4]) > 4.0 * ov.cell_edge(polys, sid)
    with world_of(bodies, sid, polys) as w:
        scene = sm.Scene(bodies, sid, polys)
        q, bad = sweep_families(rng, bodies, sid, polys, 192, shapes=[0, 1, 2])
        hits = check_three_ways(w, scene, q)
        found = hits["body"] != capi.NO_HIT
        assert set(hits["feature"][found]) == FEATURES and np.sum(found) > 60
        # the large volumes come in from outside the cloud
        start = rng.uniform(0.0, 8.0, (24, 3))
        d = unit(rng.normal(size=(24, 3)))
        big = capi.sweeps(start - d * 30.0, ov.unit_quaternions(rng, 24), d, np.where(np.arange(24) % 3 == 0, 4, 3), max_distance=40.0)
        hits = check_three_ways(w, scene, big)
        assert (hits["body"] != capi.NO_HIT).all() and (hits["distance"] > 0.0).all()


def test_a_sparse_hashed_world():
    bodies, sid = ov.sparse_world()
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(161)
    q, bad = sweep_families(rng, bodies, sid, polys, 256)
    with world_of(bodies, sid, polys, capi.MODE_FUSED) as w:
        hits = check_three_ways(w, sm.Scene(bodies, sid, polys), q)
    assert np.mean(hits["body"] != capi.NO_HIT) > 0.15


def test_a_one_body_world_and_a_world_inside_one_cell():
    polys = [capi.polytope(capi.SHAPE_CUBE)]                        # cubes only: the 16-lane groups
    rng = np.random.default_rng(171)
    one, sid1 = capi.scene_generate(capi.SCENE_BOXES, 2, 1)
    one[0, 31:34] = [0.3, -0.2, 1.0]
    edge = ov.cell_edge(polys, sid1)
    few, sid6 = capi.scene_generate(capi.SCENE_BOXES, 3, 6)
    few[:, 31:34] = 10.5 * edge + rng.uniform(-0.02, 0.02, (6, 3)) * edge       # every sphere well inside the cell (10, 10, 10)
    few[:, 34:38] = ov.unit_quaternions(rng, 6)
    for bodies, sid in ((one, sid1), (few, sid6)):
        centre = bodies[:, 31:34] + bodies[:, 28:31]
        start = centre[rng.integers(0, len(bodies), 40)] + unit(rng.normal(size=(40, 3))) * rng.uniform(0.0, 4.0, (40, 1))
        aim = centre[rng.integers(0, len(bodies), 40)] + rng.normal(size=(40, 3)) * 1.2
        q = capi.sweeps(start, ov.unit_quaternions(rng, 40), aim - start, 0, max_distance=rng.choice([0.25, 1.0, 2.0, np.inf], 40))
        with world_of(bodies, sid, polys) as w:
            hits = check_three_ways(w, sm.Scene(bodies, sid, polys), q)
        found = hits["body"] != capi.NO_HIT
        assert 10 < np.sum(found) and np.sum(~found) > 2


def test_bodies_around_the_origin_and_in_the_negative_octant():
    """Cell coordinates of either sign: bodies whose spheres contain the origin are binned in the cells -1 .. 0 on all three axes,
    others lie wholly at negative coordinates.  Sweeps start within a few cells of them."""
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(211)
    n = 96
    bodies, sid = capi.scene_generate(KIND, 4, n)
    bodies[:, 34:38] = ov.unit_quaternions(rng, n)
    bodies[:, 31:34] = rng.uniform(-6.0, 2.0, (n, 3))
    bodies[:8, 31:34] = rng.uniform(-0.2, 0.2, (8, 3))               # around the origin
    bodies[:8, 31:34] -= np.array([capi.rigid_frame(row)[:3] - row[31:34] for row in bodies[:8]])   # (the frame's origin, not `position`)
    bodies[:8, 31:34] -= np.array([np.asarray(rm.rotate(tuple(bodies[i, 34:38]), tuple(float(x) for x in polys[int(sid[i])]["centroid"]))) for i in range(8)])
    scene = sm.Scene(bodies, sid, polys)
    edge = ov.cell_edge(polys, sid)
    cells_lo = np.floor((scene.centres - scene.body_radius[:, None]) / edge)
    cells_hi = np.floor((scene.centres + scene.body_radius[:, None]) / edge)
    straddle = ((cells_lo == -1) & (cells_hi == 0)).all(axis=1)
    assert straddle[:8].all() and (cells_hi < 0).all(axis=1).sum() > 10
    # at the bodies around the origin from a few cells away, from every side; then the families over the whole cloud
    m = 96
    target = scene.centres[rng.integers(0, 8, m)] + rng.normal(size=(m, 3)) * 0.3
    start = target + unit(rng.normal(size=(m, 3))) * rng.uniform(1.0, 4.0, (m, 1)) * edge
    aimed = capi.sweeps(start, ov.unit_quaternions(rng, m), target - start, rng.integers(0, len(polys), m), max_distance=rng.choice([1.0, 2.0, np.inf], m),
                        ignore=np.where(np.arange(m) % 3 == 0, capi.NO_HIT, rng.integers(8, n, m)))
    aimed["mask"] = 1                                                # bodies from 8 on are in no group of the mask: a clear way to the origin
    groups = np.where(np.arange(n) < 8, 1, 2).astype(np.uint32)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    with world_of(bodies, sid, polys) as w:
        w.set_collision_filters(filters)
        masked_scene = sm.Scene(bodies, sid, polys, groups)
        hits = check_three_ways(w, masked_scene, aimed, MASKED)
        assert np.sum(hits["body"] < 8) > 60 and np.sum(hits["feature"][hits["body"] < 8] != capi.SWEEP_INITIAL) > 40
        q, _ = sweep_families(rng, bodies, sid, polys, 192)
        hits = check_three_ways(w, masked_scene, q)
        assert np.sum(hits["body"] != capi.NO_HIT) > 60 and np.sum(hits["body"] < 8) > 4


def test_ignore_body_and_masks():
    bodies, sid = ov.pile(1024)
    polys = capi.scene_polytopes(KIND)
    n = len(bodies)
    groups = (1 << (np.arange(n) % 3)).astype(np.uint32)
    groups[5::7] = 0                                                # bodies of no group answer unmasked sweeps only
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    rng = np.random.default_rng(181)
    with ov.stepped(bodies, sid, polys, 1, 10) as w:
        state = w.download()
        base, bad = sweep_families(rng, state, sid, polys, 128)
        unfiltered = sm.Scene(state, sid, polys)
        q = base.copy()
        q["mask"] = 4
        got = check_three_ways(w, unfiltered, q, MASKED)             # no filters set: every body is in group ~0
        assert same_hits(got, unfiltered.sweep(q))
        w.set_collision_filters(filters)
        scene = sm.Scene(state, sid, polys, groups)
        plain = check_three_ways(w, scene, base)
        found = plain["body"] != capi.NO_HIT
        assert np.any(groups[plain["body"][found]] == 0)
        # the winner of every sweep, ignored: the next body answers, later or at the same t with a larger index
        again = base.copy()
        again["ignore_body"] = plain["body"]
        second = check_three_ways(w, scene, again)
        assert (second["body"][found] != plain["body"][found]).all()
        free = found & (base["ignore_body"] == capi.NO_HIT)          # (a sweep that ignored somebody else lets that body back in)
        assert free.sum() > 30 and (second["distance"][free] >= plain["distance"][free]).all()
        for mask in (1, 2, 4, 3, 0):
            q = base.copy()
            q["mask"] = mask
            hits = check_three_ways(w, scene, q, MASKED)
            got = hits["body"] != capi.NO_HIT
            assert np.all(groups[hits["body"][got]] & mask) and (mask == 0) == (not got.any())
            assert same_hits(w.sweep(q), plain)                     # without the flag the mask field is ignored
        mixed = base.copy()
        mixed["mask"] = rng.integers(0, 8, len(base))
        check_three_ways(w, scene, mixed, MASKED)


def test_eight_and_nine_sweeps():
    """Either side of XPBD_SWEEP_BRUTE_FORCE_SWEEPS: eight sweeps take the brute-force path whatever the flags, nine the grid."""
    assert capi.SWEEP_BRUTE_FORCE_SWEEPS == 8
    bodies, sid = ov.pile(600)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(191)
    with world_of(bodies, sid, polys) as w:
        q, _ = sweep_families(rng, bodies, sid, polys, 64)
        q = q[8:17]                                                 # sweeps across the pile
        scene = sm.Scene(bodies, sid, polys)
        nine = check_three_ways(w, scene, q)
        eight = check_three_ways(w, scene, q[:8])
        assert same_hits(eight, nine[:8]) and (nine["body"] != capi.NO_HIT).sum() >= 4
        assert same_hits(w.sweep(q[:1]), nine[:1]) and len(w.sweep(q[:0])) == 0


def test_the_device_variant_equals_the_host_variant():
    """In a fresh child process that imports torch first (the library then binds to the HIP runtime torch carries)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "sweep_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"grid": True, "brute": True, "few": True, "guard": True, "hits": True}


def test_ray_casts_overlaps_and_sweeps_share_scratch_that_grows_under_use():
    """One world answers a ray cast, an overlap and a sweep in turn, batches growing, then shrinking again: every call finds
    scratch and staging that another kind sized, and grows or reuses it.  Each answer equals, bit for bit, that of the same call
    on a fresh world with the same bodies.  300 bodies: above the 256 floor of the table size, two blocks."""
    n = 300
    bodies, sid = ov.pile(n)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(183)
    centre = bodies[:, 31:34] + bodies[:, 28:31]
    r = capi.rays(centre[rng.integers(0, n, 400)] + [0.0, 0.0, 50.0], [[0.0, 0.0, -1.0]])
    q = ov.query_families(rng, bodies, sid, polys, 200)
    s, _ = sweep_families(rng, bodies, sid, polys, 640)
    at = 200 // 6 + 1
    calls = [("raycast", r[:8], 0), ("overlap", q[at:at + 8:2], 0), ("sweep", s[80:88], 0), ("raycast", r[:100], 0), ("overlap", q, 0),
             ("sweep", s[:320], 0), ("raycast", r, 0), ("sweep", s, 0), ("sweep", s, BRUTE), ("overlap", q, capi.OVERLAP_BRUTE_FORCE)]
    calls += calls[:3]

    def ask(w, kind, batch, flags):
        if kind == "raycast":
            hits = w.raycast(batch, flags)
            return hits.view(np.uint8), int(np.sum(hits["body"] != capi.NO_HIT))
        if kind == "sweep":
            hits = w.sweep(batch, flags)
            return hits.view(np.uint8), int(np.sum(hits["body"] != capi.NO_HIT))
        offsets, hits = w.overlap(batch, flags)
        return np.concatenate([offsets.view(np.uint8), hits.view(np.uint8)]), len(hits)

    with world_of(bodies, sid, polys) as w:
        got = [ask(w, *call) for call in calls]
    for call, (answer, found) in zip(calls, got):
        with world_of(bodies, sid, polys) as fresh:
            want = ask(fresh, *call)
        assert found >= 4 and ov.same_bits(answer, want[0]), call[0]


def test_a_sweep_has_no_side_effects():
    bodies, sid = ov.pile(2048)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(15)
    results = []
    for ask in (False, True):
        w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=True)
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        w.set_contact_report(True)
        for f in range(12):
            w.step(DT, 10)
            if ask:
                q, _ = sweep_families(rng, bodies, sid, polys, 96)
                w.sweep(q)
                w.sweep(q[:4], BRUTE)
        results.append((w.download(), w.contacts(), w.contact_masks(10), np.array(w.contact_stats(), dtype=np.uint64),
                        np.array(w.contact_report_counts(), dtype=np.uint64)))
        w.close()
    for a, b in zip(*results):
        assert ov.same_bits(np.asarray(a), np.asarray(b))
    assert results[0][4][0] > 0


def test_sweeps_and_overlap_queries_agree_about_the_start_pose():
    """Random poses in generic position (no exact touch): every body the overlap query lists for a volume at its start pose makes
    the sweep return distance 0, and every sweep that reports an initial overlap finds its body in that list."""
    bodies, sid = ov.pile()
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(201)
    with ov.stepped(bodies, sid, polys, 1, 10) as w:
        state = w.download()
        centre = state[:, 31:34] + state[:, 28:31]
        n = 256
        pick = rng.integers(0, len(state), n)
        pos = centre[pick] + rng.normal(size=(n, 3)) * 0.7
        rot, shape = ov.unit_quaternions(rng, n), rng.integers(0, len(polys), n)
        offsets, listed = w.overlap(capi.overlap_queries(pos, rot, shape))
        hits = w.sweep(capi.sweeps(pos, rot, unit(rng.normal(size=(n, 3))), shape, max_distance=rng.uniform(0.0, 2.0, n)))
        counts = np.diff(offsets.astype(np.int64))
        assert np.sum(counts > 0) > 60 and np.sum(counts == 0) > 20
        initial = (hits["body"] != capi.NO_HIT) & (hits["feature"] == capi.SWEEP_INITIAL)
        assert (initial == (counts > 0)).all()
        for k in np.nonzero(counts > 0)[0]:
            mine = listed["body"][offsets[k]:offsets[k + 1]]
            assert hits["distance"][k] == 0.0 and hits["body"][k] == mine[0]     # equal t: the smallest index
            # ... and ignoring the listed bodies one by one walks down the list
            for b in mine[:3] if k < 64 else []:
                one = capi.sweeps(pos[k], rot[k], [0.0, 0.0, 1.0], shape[k], max_distance=0.0, ignore=b)
                rest = [x for x in mine if x != b]
                got = w.sweep(one)[0]
                assert got["body"] == (rest[0] if rest else capi.NO_HIT)


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_the_sharded_world_equals_the_single_world(n_ranks):
    n, frames, substeps = 4096, 6, 10
    bodies, sid = capi.scene_pile(KIND, 1, n, 1.4, 4)
    polys = capi.scene_polytopes(KIND)
    groups = (1 << (np.arange(n) % 3)).astype(np.uint32)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    single = ov.stepped(bodies, sid, polys, frames, substeps)
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(polys)
        mw.upload(bodies, sid, 0, n)
        for _ in range(frames):
            mw.step(DT, substeps)
        mw.replan()
        state = single.download()
        assert ov.same_bits(mw.download(), state)
        q, _ = sweep_families(np.random.default_rng(120 + n_ranks), state, sid, polys, 256)
        want = single.sweep(q)
        assert np.sum(want["body"] != capi.NO_HIT) > 100 and np.any(q["ignore_body"] != capi.NO_HIT)
        assert same_hits(mw.sweep(q), want)
        assert same_hits(mw.sweep(q, BRUTE), want)
        assert same_hits(mw.sweep(q[32:35]), single.sweep(q[32:35]))
        single.set_collision_filters(filters)
        mw.set_collision_filters(filters)
        q["mask"] = np.random.default_rng(3).integers(0, 8, len(q))
        masked = single.sweep(q, MASKED)
        assert not same_hits(masked, want) and same_hits(mw.sweep(q, MASKED), masked)
    single.close()


def raw_sweep(w, q, fn=None, flags=0, hits=True, sweeps=True):
    """One call of the C entry point: (rc, hits) with guard values in everything it may not touch."""
    fn = fn or capi.hip_lib().xpbd_world_sweep
    out = np.zeros(len(q) + 2, dtype=capi.SWEEP_HIT_DTYPE)
    out["body"] = 0xCDCDCDCD
    rc = fn(w._h, q.ctypes.data if sweeps else None, len(q), flags, out.ctypes.data if hits else None)
    return rc, out


def test_argument_errors_leave_the_outputs_untouched():
    bodies, sid = ov.pile(64)
    polys = capi.scene_polytopes(KIND)
    L = capi.hip_lib()
    q = capi.sweeps(bodies[:2, 31:34] + [0.0, 0.0, 3.0], [IDENT], [0.0, 0.0, -1.0], [0, 1])

    def untouched(rc, out):
        return rc == capi.E_INVALID and (out["body"] == 0xCDCDCDCD).all() and not out["distance"].any()

    def cases(w, fn):
        rc, out = raw_sweep(w, q, fn)
        assert rc == capi.OK and (out["body"][:2] != 0xCDCDCDCD).all() and (out["body"][2:] == 0xCDCDCDCD).all()
        assert untouched(*raw_sweep(w, q, fn, flags=4)) and b"unknown flags" in L.xpbd_last_error()
        assert untouched(*raw_sweep(w, q, fn, sweeps=False)) and raw_sweep(w, q, fn, hits=False)[0] == capi.E_INVALID
        bad = q.copy()
        bad["reserved"][1] = 1
        assert untouched(*raw_sweep(w, bad, fn)) and b"reserved" in L.xpbd_last_error()
        bad = q.copy()
        bad["shape"][1] = len(polys)                                 # no error: that sweep hits nothing
        rc, out = raw_sweep(w, bad, fn)
        assert rc == capi.OK and out["body"][1] == capi.NO_HIT and out["body"][0] != capi.NO_HIT
        assert fn(w._h, None, 0, 0, None) == capi.OK                 # n_sweeps = 0

    with capi.World(mode=capi.MODE_CONTACTS) as w:
        assert untouched(*raw_sweep(w, q)) and b"set_polytopes" in L.xpbd_last_error()       # no polytopes
        w.set_polytopes(polys)
        assert untouched(*raw_sweep(w, q)) and b"no bodies" in L.xpbd_last_error()           # no bodies
        w.upload(bodies, sid)
        cases(w, L.xpbd_world_sweep)
        dev = L.xpbd_world_sweep_device                             # (its checks run before it touches any pointer)
        assert dev(w._h, None, 2, 0, None) == capi.E_INVALID and dev(w._h, None, 0, 8, None) == capi.E_INVALID
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL) as mw:
        fn = L.xpbd_multi_world_sweep
        assert untouched(*raw_sweep(mw, q, fn)) and b"set_polytopes" in L.xpbd_last_error()
        mw.set_polytopes(polys)
        assert untouched(*raw_sweep(mw, q, fn)) and b"no bodies" in L.xpbd_last_error()
        mw.upload(bodies, sid, 0, len(bodies))
        cases(mw, fn)
