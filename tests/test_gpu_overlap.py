"""Overlap queries on the device (include/xpbd.h, "Overlap queries"): the grid path, the brute-force path and the independent
model (tests/overlap_model.py) agree bit for bit in the offsets and in every field of every hit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import overlap_model as om
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
BRUTE, MASKED = capi.OVERLAP_BRUTE_FORCE, capi.OVERLAP_MASKED
KIND = capi.SCENE_MIXED_DROP
IDENT = [1.0, 0.0, 0.0, 0.0]


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_answer(got, want):
    return same_bits(got[0], want[0]) and got[1].dtype.itemsize == want[1].dtype.itemsize and same_bits(got[1].view(np.uint8), want[1].view(np.uint8))


def unit_quaternions(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def frames_of(state):
    return np.array([capi.rigid_frame(row) for row in state])        # Rigid::frame: origin xyz, rotation s x y z


def cell_edge(polys, sid):
    return 2.0 * max(om.shape_radius(polys[int(s)]) for s in np.unique(sid)) * (1.0 + 1e-6)


def query_families(rng, state, sid, polys, n, graze=False):
    """n queries, six families of equal share, around the bodies of `state`."""
    k = n // 6
    frames = frames_of(state)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0) - 0.5, centre.max(axis=0) + 0.5
    shapes = lambda m: rng.integers(0, len(polys), m)
    parts = []
    # random pose, random shape, inside the pile's box
    parts.append(capi.overlap_queries(rng.uniform(lo, hi, (k, 3)), unit_quaternions(rng, k), shapes(k)))
    # the exact pose and shape of a resident body, with and without ignoring it; of bodies with a neighbour within reach of
    # their bounding spheres where there are any, so that resting contacts and near misses are among the answers
    radius = np.array([om.shape_radius(polys[int(s)]) for s in sid])
    gap = np.linalg.norm(centre[:, None, :] - centre[None, :, :], axis=2) - (radius[:, None] + radius[None, :])
    np.fill_diagonal(gap, np.inf)
    with np.errstate(invalid="ignore"):
        close = np.nonzero(gap.min(axis=1) < 0.0)[0]
    pick = rng.choice(close, k) if len(close) else rng.integers(0, len(state), k)
    ignore = np.where(np.arange(k) % 2 == 0, pick, capi.NO_HIT)
    parts.append(capi.overlap_queries(frames[pick, :3], frames[pick, 3:], sid[pick], ignore=ignore))
    # poses displaced from a body by a small fraction of its radius
    pick = rng.integers(0, len(state), k)
    shift = rng.normal(size=(k, 3)) * (0.05 * radius[pick])[:, None]
    near = capi.overlap_queries(frames[pick, :3] + shift, frames[pick, 3:], sid[pick])
    if graze:
        # ... a quarter of them instead a unit cube (shape 0, spanning [0, 1]^3) set down on the highest vertex of the body, half a
        # millimetre deep: a near-touching pair whatever the bodies do among themselves
        import raycast_model as rm
        for j in range(0, k, 4):
            i = int(pick[j])
            v = np.asarray(polys[int(sid[i])]["vertices"], dtype=np.float64)
            world = np.array(rm.rotate(tuple(frames[i, 3:]), tuple(v.T))).T + frames[i, :3]
            top = world[np.argmax(world[:, 2])]
            near[j] = capi.overlap_queries([top - [0.5, 0.5, 5.0e-4]], [IDENT], 0)[0]
    parts.append(near)
    # poses well outside the pile
    away = rng.normal(size=(k, 3))
    away = away / np.linalg.norm(away, axis=1, keepdims=True) * (np.linalg.norm(hi - lo) + 10.0)
    parts.append(capi.overlap_queries(0.5 * (lo + hi) + away, unit_quaternions(rng, k), shapes(k)))
    # axis-aligned poses whose sphere centres lie on multiples of the cell edge
    edge = cell_edge(polys, sid)
    sh = shapes(k)
    centroid = np.array([polys[int(s)]["centroid"] for s in sh])
    parts.append(capi.overlap_queries(np.round(rng.uniform(lo, hi, (k, 3)) / edge) * edge - centroid, [IDENT], sh))
    # frames that are not finite
    rest = n - sum(len(p) for p in parts)
    bad = capi.overlap_queries(rng.uniform(lo, hi, (rest, 3)), unit_quaternions(rng, rest), shapes(rest))
    for j in range(rest):
        field, comp = ("position", j % 3) if j % 2 else ("rotation", j % 4)
        bad[field][j, comp] = (np.nan, np.inf, -np.inf)[j % 3]
    parts.append(bad)
    return np.concatenate(parts)


def pile(n=2048, seed=7):
    return capi.scene_pile(KIND, seed, n, 1.4, 2)


def stepped(bodies, sid, polys, frames, substeps=10, mode=capi.MODE_CONTACTS, **kw):
    w = capi.World(mode=mode, **kw)
    w.set_polytopes(polys)
    w.upload(bodies, sid)
    for _ in range(frames):
        w.step(DT, substeps)
    return w


def check_three_ways(w, scene, q, flags=0, census=None):
    want = scene.overlap(q, masked=bool(flags & MASKED), census=census)
    grid, brute = w.overlap(q, flags), w.overlap(q, flags | BRUTE)
    assert same_answer(grid, brute)
    assert same_answer(grid, want)
    for a, b in zip(want[0][:-1], want[0][1:]):
        assert np.all(np.diff(want[1]["body"][a:b].astype(np.int64)) > 0)
    return want


@pytest.mark.parametrize("mode", [capi.MODE_CONTACTS, capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
def test_grid_brute_force_and_model_agree_on_a_mixed_pile(mode):
    bodies, sid = pile()
    polys = capi.scene_polytopes(KIND)
    with stepped(bodies, sid, polys, 30, mode=mode) as w:
        state = w.download()
        q = query_families(np.random.default_rng(40 + mode), state, sid, polys, 384, graze=True)
        census = {}
        offsets, hits = check_three_ways(w, om.Scene(state, sid, polys), q, census=census)
    counts = np.diff(offsets.astype(np.int64))
    assert np.mean(counts > 0) >= 0.25 and np.mean(counts == 0) >= 0.10
    assert set(hits["feature"]) == {capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES}
    assert np.sum(-hits["separation"] < 1e-3) >= 8                 # near-touching pairs, not only gross overlap
    assert census["sat_rejects"] > 0                               # spheres overlap, the SAT separates: step 3 rejects too
    assert (hits["separation"] < 0.0).all()


def test_wide_groups_on_random_convex_hulls():
    """Shapes above 16 vertices take the 64-lane groups and edge-direction tables too large to stage."""
    import hull_util as hu
    raw = [hu.random_hull(7, 18, 0.6), hu.random_hull(8, 16, 0.5), hu.random_hull(9, 10, 0.4)]
    polys = [hu.as_capi(*h) for h in raw]
    n = 512
    rng = np.random.default_rng(51)
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, 5, n)
    bodies[:, 31:34] = rng.uniform(0.0, 6.0, (n, 3))
    bodies[:, 34:38] = unit_quaternions(rng, n)
    bodies[:, 28:31] = 0.0                                          # the hulls are centred: com = 0
    sid = (np.arange(n) % 3).astype(np.uint32)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        q = query_families(rng, bodies, sid, polys, 192)
        offsets, hits = check_three_ways(w, om.Scene(bodies, sid, polys), q)
    assert max(len(p["vertices"]) for p in polys) > 16 and offsets[-1] > 200
    assert set(hits["feature"]) == {capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES}


def test_a_large_volume_and_segments_longer_than_the_sort_stage():
    n = 4096
    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, 1, n, 2.0, 16)    # 16 x 16 boxes a layer: 32 m x 32 m x 40 m
    polys = [capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, 40.0)]    # no body uses the second
    centre = bodies[:, 31:34] + bodies[:, 28:31]
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    assert (hi - lo).max() < 39.0                                   # a 40 m box can hold every centre
    # a box over a corner of the pile, and one around the whole world that ignores one body
    q = capi.overlap_queries([lo + [12.0, 12.0, -1.0], 0.5 * (lo + hi) - 20.0], [IDENT], [1], ignore=[capi.NO_HIT, 2500])
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        offsets, hits = check_three_ways(w, om.Scene(bodies, sid, polys), q)
    counts = np.diff(offsets.astype(np.int64))
    assert 40.0 / cell_edge(polys, sid) > 20.0                      # the volume spans many cells per axis
    assert capi.OVERLAP_SORT_STAGE < counts[0] < n                  # longer than the sort's LDS stage, and not everybody
    assert list(hits["body"][offsets[1]:]) == [i for i in range(n) if i != 2500]


def sparse_world(n=4096):
    """Bodies spread over a 4 km cube: far more cells than the table has buckets, so the grid is hashed."""
    rng = np.random.default_rng(3)
    bodies, sid = capi.scene_generate(KIND, 3, n)
    bodies[:, 31:34] = rng.uniform(-2000.0, 2000.0, (n, 3))
    # ... and a few clusters, so that volumes of body size touch something
    for c in range(64):
        members = rng.integers(0, n, 6)
        bodies[members, 31:34] = bodies[members[0], 31:34] + rng.uniform(-0.6, 0.6, (6, 3))
    return bodies, sid


def test_a_sparse_hashed_world():
    bodies, sid = sparse_world()
    polys = capi.scene_polytopes(KIND) + [capi.polytope(capi.SHAPE_CUBE, 1500.0)]   # the last: more cells than any walk covers
    rng = np.random.default_rng(61)
    q = query_families(rng, bodies, sid, polys[:3], 384)
    q = np.concatenate([q, capi.overlap_queries([[-700.0, -800.0, -750.0], [100.0, 200.0, 300.0]], [IDENT], [3])])
    with capi.World(mode=capi.MODE_FUSED) as w:
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        offsets, hits = check_three_ways(w, om.Scene(bodies, sid, polys), q)
    counts = np.diff(offsets.astype(np.int64))
    assert np.mean(counts[:384] > 0) > 0.2 and counts[384] > 50 and counts[385] > 50


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def centred_queries(rng, polys, at, shape):
    """Queries of random rotation whose bounding-sphere centres (the shapes' centroids) lie at the points `at`."""
    import raycast_model as rm
    rot = unit_quaternions(rng, len(at))
    shape = np.broadcast_to(shape, len(at))
    off = np.array([rm.rotate(tuple(r), tuple(float(x) for x in polys[int(s)]["centroid"])) for r, s in zip(rot, shape)])
    return capi.overlap_queries(at - off, rot, shape)


def put_centres(bodies, sid, polys, rows, at):
    """Move the bodies `rows` so that the centres of their bounding spheres lie at the points `at`."""
    import raycast_model as rm
    bodies[rows, 31:34] = at
    bodies[rows, 31:34] -= np.array([capi.rigid_frame(row)[:3] - row[31:34] for row in bodies[rows]])   # (the frame's origin, not `position`)
    bodies[rows, 31:34] -= np.array([rm.rotate(tuple(bodies[i, 34:38]), tuple(float(x) for x in polys[int(sid[i])]["centroid"])) for i in rows])


def test_a_one_body_world_and_a_world_inside_one_cell():
    polys = [capi.polytope(capi.SHAPE_CUBE)]                        # cubes only: the 16-lane groups
    rng = np.random.default_rng(271)
    one, sid1 = capi.scene_generate(capi.SCENE_BOXES, 2, 1)
    one[0, 31:34] = [0.3, -0.2, 1.0]
    edge = cell_edge(polys, sid1)
    few, sid6 = capi.scene_generate(capi.SCENE_BOXES, 3, 6)
    few[:, 34:38] = unit_quaternions(rng, 6)
    # a sphere is narrower than a cell by 1e-6 of an edge: centres within 2e-7 of the middle of the cell (10, 10, 10) keep every
    # sphere inside it, the pad of 1e-7 radii included -- a grid of one cell
    put_centres(few, sid6, polys, range(6), 10.5 * edge + rng.uniform(-2e-7, 2e-7, (6, 3)) * edge)
    for bodies, sid in ((one, sid1), (few, sid6)):
        scene = om.Scene(bodies, sid, polys)
        if len(bodies) > 1:
            reach = scene.body_radius[:, None] * (1.0 + 1e-7)
            assert (np.floor((scene.centres - reach) / edge) == 10).all() and (np.floor((scene.centres + reach) / edge) == 10).all()
        # on the bodies and up to two cells away from them: the centres of a hit lie within 2 * radius, just over one edge
        at = scene.centres[rng.integers(0, len(bodies), 40)] + unit(rng.normal(size=(40, 3))) * rng.uniform(0.0, 2.0, (40, 1)) * edge
        q = centred_queries(rng, polys, at, 0)
        with capi.World(mode=capi.MODE_CONTACTS) as w:
            w.set_polytopes(polys)
            w.upload(bodies, sid)
            offsets, hits = check_three_ways(w, scene, q)
        counts = np.diff(offsets.astype(np.int64))
        assert np.sum(counts > 0) > 8 and np.sum(counts == 0) > 8
        assert set(counts) <= set(range(len(bodies) + 1)) and counts.max() == len(bodies)


def test_bodies_around_the_origin_and_in_the_negative_octant():
    """Cell coordinates of either sign: bodies whose spheres contain the origin are binned in the cells -1 .. 0 on all three axes,
    others lie wholly at negative coordinates.  Volumes of body size and volumes several cells wide, whose boxes of cells span
    the change of sign, unmasked and masked."""
    kinds = capi.scene_polytopes(KIND)
    polys = kinds + [capi.polytope(capi.SHAPE_CUBE, 2.5)]           # the last: larger than a cell, no body uses it
    big = len(kinds)
    rng = np.random.default_rng(311)
    n = 96
    bodies, sid = capi.scene_generate(KIND, 4, n)
    bodies[:, 34:38] = unit_quaternions(rng, n)
    bodies[:, 31:34] = rng.uniform(-6.0, 2.0, (n, 3))
    put_centres(bodies, sid, polys, range(8), rng.uniform(-0.2, 0.2, (8, 3)))   # around the origin
    groups = np.where(np.arange(n) < 8, 1, 2).astype(np.uint32)
    scene = om.Scene(bodies, sid, polys, groups)
    edge = cell_edge(polys, sid)
    cells_lo = np.floor((scene.centres - scene.body_radius[:, None]) / edge)
    cells_hi = np.floor((scene.centres + scene.body_radius[:, None]) / edge)
    straddle = ((cells_lo == -1) & (cells_hi == 0)).all(axis=1)
    negative = (cells_hi < 0).all(axis=1)
    assert straddle[:8].all() and negative.sum() > 10
    assert 2.0 * om.shape_radius(polys[big]) > 2.0 * edge            # its sphere's box of cells is 3 to 4 cells wide
    # body-sized volumes at the bodies around the origin; large ones whose boxes hold the origin's cells; the families over the
    # whole cloud, with volumes of every shape
    q = np.concatenate([centred_queries(rng, polys, scene.centres[rng.integers(0, 8, 48)] + rng.normal(size=(48, 3)) * 0.4, rng.integers(0, big, 48)),
                        centred_queries(rng, polys, rng.uniform(-0.5, 0.5, (32, 3)), big),
                        centred_queries(rng, polys, rng.uniform(-6.0, -1.0, (24, 3)), big),
                        query_families(rng, bodies, sid, polys, 96)])
    assert len(q) == 200
    q["ignore_body"][1:48:3] = rng.integers(0, 8, 16)
    q["mask"] = rng.integers(0, 4, len(q))
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        w.set_collision_filters(filters)
        offsets, hits = check_three_ways(w, scene, q)
        counts = np.diff(offsets.astype(np.int64))
        assert np.sum(hits["body"] < 8) > 100 and np.sum(negative[hits["body"]]) > 100
        # (the eight centres lie within 0.35 of the origin and a large volume's within 0.87, less than the 1.25 from its centre to a face)
        assert (counts[48:80] >= 8).all()                            # around the origin a large volume holds all eight
        assert np.sum(counts > 0) > 100 and np.sum(counts == 0) > 20
        m_offsets, m_hits = check_three_ways(w, scene, q, MASKED)
        assert 50 < len(m_hits) < len(hits) and np.all(groups[m_hits["body"]] & np.repeat(q["mask"], np.diff(m_offsets.astype(np.int64))))
        assert np.sum(m_hits["body"] < 8) > 30 and np.sum(negative[m_hits["body"]]) > 30


def test_masks():
    bodies, sid = pile(1024)
    polys = capi.scene_polytopes(KIND)
    n = len(bodies)
    groups = (1 << (np.arange(n) % 3)).astype(np.uint32)
    groups[5::50] = 0                                               # bodies of no group answer unmasked queries only
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    rng = np.random.default_rng(71)
    with stepped(bodies, sid, polys, 20) as w:
        state = w.download()
        base = query_families(rng, state, sid, polys, 96)
        unfiltered = om.Scene(state, sid, polys)
        q = base.copy()
        q["mask"] = 4
        got = check_three_ways(w, unfiltered, q, MASKED)             # no filters set: every body is in group ~0
        assert same_answer(got, unfiltered.overlap(q))
        w.set_collision_filters(filters)
        scene = om.Scene(state, sid, polys, groups)
        plain = check_three_ways(w, scene, base)
        assert np.any(groups[plain[1]["body"]] == 0)
        for mask in (1, 2, 4, 3, 0):
            q = base.copy()
            q["mask"] = mask
            offsets, hits = check_three_ways(w, scene, q, MASKED)
            assert np.all(groups[hits["body"]] & mask) and (mask == 0) == (len(hits) == 0)
            assert same_answer(w.overlap(q), plain)                 # without the flag the mask field is ignored
        mixed = base.copy()
        mixed["mask"] = rng.integers(0, 8, len(base))
        check_three_ways(w, scene, mixed, MASKED)


def raw_overlap(w, q, cap, hits=True, fn=None):
    """One call of the C entry point: (rc, offsets, hits, n_out) with guard values in everything it may not touch."""
    fn = fn or capi.hip_lib().xpbd_world_overlap
    offsets = np.full(len(q) + 1, 0xABABABAB, dtype=np.uint32)
    out = np.zeros(cap + 4, dtype=capi.OVERLAP_HIT_DTYPE)
    out["body"] = 0xCDCDCDCD
    total = capi.C.c_uint32(0xEFEFEFEF)
    rc = fn(w._h, q.ctypes.data if len(q) else None, len(q), 0, offsets.ctypes.data, out.ctypes.data if hits else None, cap, capi.C.byref(total))
    return rc, offsets, out, total.value


def capacity_cases(w, q, fn=None):
    offsets, hits = w.overlap(q)
    total = len(hits)
    assert total > 8
    rc, off, _, n_out = raw_overlap(w, q, 0, hits=False, fn=fn)       # a pure count
    assert rc == capi.E_CAPACITY and n_out == total and same_bits(off, offsets)
    rc, off, out, n_out = raw_overlap(w, q, total - 1, fn=fn)
    assert rc == capi.E_CAPACITY and n_out == total and same_bits(off, offsets)
    assert same_bits(out[:total - 1].view(np.uint8), hits[:total - 1].view(np.uint8)) and (out["body"][total - 1:] == 0xCDCDCDCD).all()
    cut = int(offsets[np.argmax(np.diff(offsets.astype(np.int64)))]) + 1   # inside the longest segment
    rc, off, out, n_out = raw_overlap(w, q, cut, fn=fn)
    assert rc == capi.E_CAPACITY and same_bits(out[:cut].view(np.uint8), hits[:cut].view(np.uint8)) and (out["body"][cut:] == 0xCDCDCDCD).all()
    rc, off, out, n_out = raw_overlap(w, q, total, fn=fn)
    assert rc == capi.OK and n_out == total and same_bits(out[:total].view(np.uint8), hits.view(np.uint8))
    rc, off, _, n_out = raw_overlap(w, q[:0], 0, hits=False, fn=fn)    # n_queries = 0
    assert rc == capi.OK and n_out == 0
    nothing = q[:2].copy()
    nothing["position"] += 1.0e4
    rc, off, _, n_out = raw_overlap(w, nothing, 0, hits=False, fn=fn)  # a count of nothing is no error
    assert rc == capi.OK and n_out == 0 and list(off) == [0, 0, 0]


def test_capacity_and_counting():
    bodies, sid = pile(1024)
    polys = capi.scene_polytopes(KIND)
    with stepped(bodies, sid, polys, 20) as w:
        q = query_families(np.random.default_rng(81), w.download(), sid, polys, 96)
        capacity_cases(w, q)


def test_the_device_variant_equals_the_host_variant():
    """In a fresh child process that imports torch first (the library then binds to the HIP runtime torch carries)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "overlap_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"grid": True, "brute": True, "short_total": True, "short_prefix": True, "short_guard": True, "hits": True}


def test_an_overlap_query_has_no_side_effects():
    bodies, sid = pile(2048)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(5)
    results = []
    for ask in (False, True):
        w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=True)
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        w.set_contact_report(True)
        for f in range(12):
            w.step(DT, 10)
            if ask:
                q = query_families(rng, bodies, sid, polys, 96)
                w.overlap(q)
                w.overlap(q[:4], BRUTE)
        results.append((w.download(), w.contacts(), w.contact_masks(10), np.array(w.contact_stats(), dtype=np.uint64),
                        np.array(w.contact_report_counts(), dtype=np.uint64)))
        w.close()
    for a, b in zip(*results):
        assert same_bits(np.asarray(a), np.asarray(b))
    assert results[0][4][0] > 0


def test_ray_casts_and_overlaps_share_scratch_that_grows_under_use():
    """One world answers a stream of calls of both kinds and both paths, small batches before large ones: every call after the
    first finds scratch and staging that the other kind sized, and grows or reuses it.  Each answer equals, bit for bit, that of
    the same call on a fresh world with the same bodies.  300 bodies: above the 256 floor of the table size, two blocks."""
    n = 300
    bodies, sid = pile(n)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(83)
    centre = bodies[:, 31:34] + bodies[:, 28:31]
    # rays: straight down onto bodies from above the pile, then random ones inside its box
    d = rng.normal(size=(300, 3))
    lo, hi = centre.min(axis=0) - 0.5, centre.max(axis=0) + 0.5
    r = np.concatenate([capi.rays(centre[rng.integers(0, n, 300)] + [0.0, 0.0, 50.0], [[0.0, 0.0, -1.0]]),
                        capi.rays(rng.uniform(lo, hi, (300, 3)), d / np.linalg.norm(d, axis=1, keepdims=True))])
    q = query_families(rng, bodies, sid, polys, 200)
    at = 200 // 6 + 1                                               # the second family: poses of resident bodies, nobody ignored
    calls = [("raycast", r[:8], capi.RAYCAST_BRUTE_FORCE), ("overlap", q[at:at + 8:2], 0), ("raycast", r, 0), ("overlap", q, BRUTE)]
    calls += calls[:2]
    assert len(r) == 600 and len(calls[1][1]) == 4

    def world():
        w = capi.World(mode=capi.MODE_CONTACTS)
        w.set_polytopes(polys)
        w.upload(bodies, sid)
        return w

    def ask(w, kind, batch, flags):
        if kind == "raycast":
            hits = w.raycast(batch, flags)
            return np.zeros(0, dtype=np.uint32), hits, int(np.sum(hits["body"] != capi.NO_HIT))
        offsets, hits = w.overlap(batch, flags)
        return offsets, hits, len(hits)

    with world() as w:
        got = [ask(w, *call) for call in calls]
    for call, (offsets, hits, found) in zip(calls, got):
        with world() as fresh:
            want = ask(fresh, *call)
        assert found >= 4 and same_answer((offsets, hits), want[:2]), call[0]


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_the_sharded_world_equals_the_single_world(n_ranks):
    n, frames, substeps = 4096, 6, 10
    bodies, sid = capi.scene_pile(KIND, 1, n, 1.4, 4)
    polys = capi.scene_polytopes(KIND)
    groups = (1 << (np.arange(n) % 3)).astype(np.uint32)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    single = stepped(bodies, sid, polys, frames, substeps)
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(polys)
        mw.upload(bodies, sid, 0, n)
        for _ in range(frames):
            mw.step(DT, substeps)
        state = single.download()
        q = query_families(np.random.default_rng(20 + n_ranks), state, sid, polys, 192)
        want = single.overlap(q)
        assert want[0][-1] > 100 and np.any(q["ignore_body"] != capi.NO_HIT)
        assert same_answer(mw.overlap(q), want)             # under the plans the steps made; then under one more
        mw.replan()
        assert mw.plan_stats()["plans"] >= 2
        assert same_bits(mw.download(), state)
        assert same_answer(mw.overlap(q), want)
        assert same_answer(mw.overlap(q, BRUTE), want)
        assert same_answer(mw.overlap(q[:3]), single.overlap(q[:3]))
        single.set_collision_filters(filters)
        mw.set_collision_filters(filters)
        q["mask"] = np.random.default_rng(3).integers(0, 8, len(q))
        masked = single.overlap(q, MASKED)
        assert masked[0][-1] < want[0][-1] and same_answer(mw.overlap(q, MASKED), masked)
        capacity_cases(mw, q, fn=capi.hip_lib().xpbd_multi_world_overlap)
    single.close()


def test_argument_errors_leave_the_outputs_untouched():
    bodies, sid = pile(64)
    polys = capi.scene_polytopes(KIND)
    L = capi.hip_lib()
    q = capi.overlap_queries(bodies[:2, 31:34], [IDENT], [0, 1])

    def untouched(rc, off, out, n_out):
        return rc == capi.E_INVALID and (off == 0xABABABAB).all() and (out["body"] == 0xCDCDCDCD).all() and n_out == 0xEFEFEFEF

    def cases(w, fn):
        assert raw_overlap(w, q, 8, fn=fn)[0] == capi.OK
        offsets = np.full(3, 0xABABABAB, dtype=np.uint32)
        out = np.zeros(8, dtype=capi.OVERLAP_HIT_DTYPE)
        total = capi.C.c_uint32(0xEFEFEFEF)
        args = lambda **kw: [w._h, kw.get("q", q.ctypes.data), 2, kw.get("flags", 0), kw.get("off", offsets.ctypes.data), kw.get("hits", out.ctypes.data),
                             kw.get("cap", 8), kw.get("n_out", capi.C.byref(total))]
        assert fn(*args(flags=4)) == capi.E_INVALID and b"unknown flags" in L.xpbd_last_error()
        assert fn(*args(q=None)) == capi.E_INVALID and fn(*args(off=None)) == capi.E_INVALID
        assert fn(*args(hits=None)) == capi.E_INVALID and fn(*args(n_out=None)) == capi.E_INVALID
        bad = q.copy()
        bad["reserved"][1] = 1
        assert fn(*args(q=bad.ctypes.data)) == capi.E_INVALID and b"reserved" in L.xpbd_last_error()
        bad = q.copy()
        bad["shape"][1] = len(polys)
        assert fn(*args(q=bad.ctypes.data)) == capi.E_INVALID and b"shape" in L.xpbd_last_error()
        assert (offsets == 0xABABABAB).all() and not out["body"].any() and total.value == 0xEFEFEFEF

    with capi.World(mode=capi.MODE_CONTACTS) as w:
        assert untouched(*raw_overlap(w, q, 8))                     # no polytopes
        assert b"set_polytopes" in L.xpbd_last_error()
        w.set_polytopes(polys)
        assert untouched(*raw_overlap(w, q, 8))                     # no bodies
        assert b"no bodies" in L.xpbd_last_error()
        w.upload(bodies, sid)
        cases(w, L.xpbd_world_overlap)
        dev = L.xpbd_world_overlap_device                           # (its checks run before it touches any pointer)
        assert dev(w._h, None, 2, 0, None, None, 0) == capi.E_INVALID and dev(w._h, None, 0, 8, None, None, 0) == capi.E_INVALID
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL) as mw:
        fn = L.xpbd_multi_world_overlap
        assert untouched(*raw_overlap(mw, q, 8, fn=fn)) and b"set_polytopes" in L.xpbd_last_error()
        mw.set_polytopes(polys)
        assert untouched(*raw_overlap(mw, q, 8, fn=fn)) and b"no bodies" in L.xpbd_last_error()
        mw.upload(bodies, sid, 0, len(bodies))
        cases(mw, fn)
