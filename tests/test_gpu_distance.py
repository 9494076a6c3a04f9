"""Distance queries on the device (include/xpbd.h, "Distance queries"): the grid path, the brute-force path and the independent
model (tests/distance_model.py) agree bit for bit in every field of every hit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_model as dm
import raycast_model as rm
import test_gpu_overlap as ov
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
BRUTE, MASKED = capi.DISTANCE_BRUTE_FORCE, capi.DISTANCE_MASKED
KIND = capi.SCENE_MIXED_DROP
IDENT = [1.0, 0.0, 0.0, 0.0]
POINT = capi.DISTANCE_POINT
FACES = (capi.FEATURE_FACE_A, capi.FEATURE_FACE_B)


def same_hits(a, b):
    return a.dtype.itemsize == b.dtype.itemsize == 96 and ov.same_bits(a.view(np.uint8), b.view(np.uint8))


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def world_vertices(state_row, frame, poly):
    v = np.asarray(poly["vertices"], dtype=np.float64)
    return np.array(rm.rotate(tuple(frame[3:]), tuple(v.T))).T + frame[:3]


def distance_families(rng, state, sid, polys, n, shapes=None):
    """n queries, eight families of equal share, around the bodies of `state`; volumes of the shapes listed (default: all).  Returns
    the records and the size of the last family, the records that can find nothing."""
    k = n // 8
    frames = ov.frames_of(state)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0) - 0.5, centre.max(axis=0) + 0.5
    span = float(np.linalg.norm(hi - lo))
    pool = np.arange(len(polys)) if shapes is None else np.asarray(shapes)
    pick_shapes = lambda m: pool[rng.integers(0, len(pool), m)]
    quats = lambda m: ov.unit_quaternions(rng, m)
    radius = np.array([dm.om.shape_radius(polys[int(s)]) for s in sid])
    parts = []
    # body-sized volumes inside the pile's box, bounded reach
    parts.append(capi.distances(rng.uniform(lo, hi, (k, 3)), quats(k), pick_shapes(k), max_distance=rng.uniform(0.05, 1.5, k)))
    # points: anywhere in the box, and inside bodies (a fraction of a radius off a body's centre), bounded and unbounded
    pick = rng.integers(0, len(state), k)
    at = np.where((np.arange(k) % 2 == 0)[:, None], rng.uniform(lo, hi, (k, 3)), centre[pick] + rng.normal(size=(k, 3)) * (0.3 * radius[pick])[:, None])
    parts.append(capi.distances(at, quats(k), POINT, max_distance=np.where(np.arange(k) % 4 < 2, rng.uniform(0.05, 1.0, k), np.inf)))
    # volumes and points outside the pile's box, no limit
    away = unit(rng.normal(size=(k, 3))) * (0.5 * span + rng.uniform(1.0, 6.0, (k, 1)))
    parts.append(capi.distances(0.5 * (lo + hi) + away, quats(k), np.where(np.arange(k) % 3 == 0, POINT, pick_shapes(k))))
    # sphere centres on cell faces: axis-aligned volumes whose centroid sits on multiples of the cell edge
    edge = ov.cell_edge(polys, sid)
    sh = pick_shapes(k)
    centroid = np.array([polys[int(s)]["centroid"] for s in sh])
    on_face = np.round(rng.uniform(lo, hi, (k, 3)) / edge) * edge - centroid
    parts.append(capi.distances(on_face, [IDENT], sh, max_distance=rng.uniform(0.2, 1.0, k) * edge))
    # a body's own pose and shape, with and without ignoring it
    pick = rng.integers(0, len(state), k)
    parts.append(capi.distances(frames[pick, :3], frames[pick, 3:], sid[pick], max_distance=rng.uniform(0.1, 1.0, k),
                                ignore=np.where(np.arange(k) % 2 == 0, pick, capi.NO_HIT)))
    # max_distance 0 (an overlap, an exact touch or nothing), from poses a fraction of a radius off a body
    pick = rng.integers(0, len(state), k)
    shift = rng.normal(size=(k, 3)) * (0.6 * radius[pick])[:, None]
    parts.append(capi.distances(frames[pick, :3] + shift, quats(k), pick_shapes(k), max_distance=0.0,
                                ignore=np.where(np.arange(k) % 4 < 2, pick, capi.NO_HIT)))
    # grazing: a unit cube (shape 0, spanning [0, 1]^3) above the highest vertex of a body, its bottom face half a millimetre clear
    # of the vertex or half a millimetre into it
    pick = rng.integers(0, len(state), k)
    graze = capi.distances(np.zeros((k, 3)), [IDENT], 0, max_distance=0.25)
    for j in range(k):
        i = int(pick[j])
        world = world_vertices(state[i], frames[i], polys[int(sid[i])])
        top = world[np.argmax(world[:, 2])]
        graze["position"][j] = top - [0.5, 0.5, -5.0e-4 if j % 2 == 0 else 5.0e-4]
    parts.append(graze)
    # records that can find nothing: frame not finite, shape outside the table, max_distance < 0 or NaN
    rest = n - sum(len(p) for p in parts)
    bad = capi.distances(frames[rng.integers(0, len(state), rest), :3], quats(rest), np.where(np.arange(rest) % 2 == 0, POINT, pick_shapes(rest)))
    for j in range(rest):
        case = j % 4
        if case == 0:
            bad["position" if j % 8 < 4 else "rotation"][j, j % 3] = (np.nan, np.inf, -np.inf)[(j // 4) % 3]
        elif case == 1:
            bad["shape"][j] = len(polys) + (j // 4) % 2 * 1000
        elif case == 2:
            bad["max_distance"][j] = -1.0e-300 if (j // 4) % 2 else -2.0
        else:
            bad["max_distance"][j] = np.nan
    parts.append(bad)
    return np.concatenate(parts), rest


def check_three_ways(w, scene, q, flags=0):
    want = scene.distance(q, masked=bool(flags & MASKED))
    grid, brute = w.distance(q, flags), w.distance(q, flags | BRUTE)
    assert same_hits(grid, brute)
    assert same_hits(grid, want)
    return want


def world_of(bodies, sid, polys, mode=capi.MODE_CONTACTS):
    w = capi.World(mode=mode)
    w.set_polytopes(polys)
    w.upload(bodies, sid)
    return w


def feature_shares(hits):
    """Among the answers at a finite distance > 0: the share through a face (either way) and through two edges."""
    apart = hits[(hits["body"] != capi.NO_HIT) & (hits["feature"] != capi.DISTANCE_OVERLAP)]
    return len(apart), float(np.isin(apart["feature"], FACES).mean()), float((apart["feature"] == capi.FEATURE_EDGES).mean())


@pytest.mark.parametrize("mode", [capi.MODE_CONTACTS, capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
def test_grid_brute_force_and_model_agree_on_a_mixed_pile(mode):
    bodies, sid = ov.pile()
    polys = capi.scene_polytopes(KIND)
    with ov.stepped(bodies, sid, polys, 1, 10, mode=mode) as w:
        state = w.download()
        q, bad = distance_families(np.random.default_rng(340), state, sid, polys, 512)
        hits = check_three_ways(w, dm.Scene(state, sid, polys), q)
    k = len(q) // 8
    found = hits["body"] != capi.NO_HIT
    assert set(hits["feature"][found]) == {capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES, capi.DISTANCE_OVERLAP}
    apart, through_faces, through_edges = feature_shares(hits)
    print("answers at a distance: %d, through a face %.3f, through two edges %.3f" % (apart, through_faces, through_edges))
    # (on the pile before its first step the model gives 0.33 and 0.67 of 199 such answers)
    assert apart > 100 and through_faces >= 0.25 and through_edges >= 0.25
    assert not found[-bad:].any() and np.mean(found) > 0.5 and np.sum(~found[:-bad]) >= 16
    miss = hits[~found]
    assert (miss["index_a"] == capi.NO_HIT).all() and (miss["index_b"] == capi.NO_HIT).all() and np.isinf(miss["distance"]).all()
    assert not miss["feature"].any() and not miss["point_a"].any() and not miss["point_b"].any() and not miss["normal"].any()
    over = hits[found & (hits["feature"] == capi.DISTANCE_OVERLAP)]
    assert not over["distance"].any() and not over["normal"].any() and (over["index_a"] == capi.NO_HIT).all()
    assert found[2 * k:3 * k].all() and (hits["distance"][2 * k:3 * k] > 0.5).all()      # from outside, unbounded: always an answer
    own = hits[4 * k + 1:5 * k:2]                                     # a body's own pose, nobody ignored: not separated from itself
    assert (own["feature"] == capi.DISTANCE_OVERLAP).all()
    assert (hits["body"][4 * k:5 * k:2] != q["ignore_body"][4 * k:5 * k:2]).all()
    graze = hits[6 * k:7 * k]
    assert np.sum(graze["feature"] == capi.DISTANCE_OVERLAP) >= k // 4 and np.sum((graze["distance"] > 0.0) & (graze["distance"] < 6.0e-4)) >= k // 4
    at_zero = hits[5 * k:6 * k]
    assert (at_zero["distance"][at_zero["body"] != capi.NO_HIT] == 0.0).all()


def random_simple_polytope(seed, n_planes=18, radius=0.5):
    """A random polytope of 2 * n_planes - 4 vertices: the intersection of n_planes half-spaces tangent to a sphere, in generic
    position, so three faces meet in every vertex (18 planes: 32 vertices, 48 edges -- a triangulated hull of 32 points has 90
    edges and 60 faces, more than the oracle's tables hold).  Faces of at most 8 vertices."""
    from scipy.spatial import HalfspaceIntersection
    rng = np.random.default_rng(seed)
    while True:
        normals = unit(rng.normal(size=(n_planes, 3)))
        try:
            pts = HalfspaceIntersection(np.hstack([normals, -radius * np.ones((n_planes, 1))]), np.zeros(3)).intersections
        except Exception:
            continue
        pts = np.unique(np.round(pts, 12), axis=0)
        if len(pts) != 2 * n_planes - 4 or np.abs(pts).max() > 4.0 * radius:
            continue
        faces = []
        for n in normals:
            on = np.nonzero(np.abs(pts @ n - radius) < 1e-9)[0]
            u = unit(np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])[None])[0]
            mid = pts[on].mean(axis=0)
            angle = np.arctan2((pts[on] - mid) @ np.cross(n, u), (pts[on] - mid) @ u)
            faces.append([int(x) for x in on[np.argsort(angle)]])
        if all(3 <= len(f) <= 8 for f in faces):
            break
    edges = sorted({tuple(sorted((f[i], f[(i + 1) % len(f)]))) for f in faces for i in range(len(f))})
    assert len(edges) == 3 * n_planes - 6
    return {"vertices": pts, "edges": np.array(edges, dtype=np.uint32), "face_offsets": np.cumsum([0] + [len(f) for f in faces]).astype(np.uint32),
            "face_indices": np.array([i for f in faces for i in f], dtype=np.uint32), "centroid": pts.mean(axis=0)}


def test_wide_groups_on_polytopes_of_32_vertices_and_a_reach_beyond_the_walk():
    """Shapes above 16 vertices take the 64-lane groups; 32 vertices fill the staging.  Against boxes and an 18-vertex triangulated
    hull.  A max_distance of six cell edges is beyond the walk (kSweepReach = 4) and looks at every body."""
    import hull_util as hu
    polys = [random_simple_polytope(5), random_simple_polytope(6, radius=0.4), capi.polytope(capi.SHAPE_CUBE), hu.as_capi(*hu.random_hull(7, 18, 0.6))]
    assert len(polys[0]["vertices"]) == len(polys[1]["vertices"]) == 32 and len(polys[0]["edges"]) == 48
    n = 384
    rng = np.random.default_rng(351)
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, 5, n)
    bodies[:, 31:34] = rng.uniform(0.0, 9.0, (n, 3))
    bodies[:, 34:38] = ov.unit_quaternions(rng, n)
    bodies[:, 28:31] = 0.0
    sid = np.where(np.arange(n) % 2 == 0, 2, np.arange(n) % 4).astype(np.uint32)       # half of them boxes
    with world_of(bodies, sid, polys) as w:
        scene = dm.Scene(bodies, sid, polys)
        q, bad = distance_families(rng, bodies, sid, polys, 192, shapes=[0, 1, 3])
        hits = check_three_ways(w, scene, q)
        found = hits["body"] != capi.NO_HIT
        assert np.sum(found) > 60 and {capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES} <= set(hits["feature"][found])
        edge = ov.cell_edge(polys, sid)
        far = capi.distances(rng.uniform(-3.0, 12.0, (24, 3)), ov.unit_quaternions(rng, 24), np.where(np.arange(24) % 3 == 0, POINT, 0), max_distance=6.0 * edge)
        near = far.copy()
        near["max_distance"] = 3.0 * edge                              # inside the walk, boxes of many cells
        for batch in (far, near):
            hits = check_three_ways(w, scene, batch)
            assert np.sum(hits["body"] != capi.NO_HIT) > 12


def test_a_sparse_hashed_world():
    bodies, sid = ov.sparse_world()
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(361)
    q, bad = distance_families(rng, bodies, sid, polys, 256)
    with world_of(bodies, sid, polys, capi.MODE_FUSED) as w:
        hits = check_three_ways(w, dm.Scene(bodies, sid, polys), q)
    assert np.mean(hits["body"] != capi.NO_HIT) > 0.15


def test_a_one_body_world_and_a_world_inside_one_cell():
    polys = [capi.polytope(capi.SHAPE_CUBE)]                        # cubes only: the 16-lane groups
    rng = np.random.default_rng(371)
    one, sid1 = capi.scene_generate(capi.SCENE_BOXES, 2, 1)
    one[0, 31:34] = [0.3, -0.2, 1.0]
    edge = ov.cell_edge(polys, sid1)
    few, sid6 = capi.scene_generate(capi.SCENE_BOXES, 3, 6)
    few[:, 31:34] = 10.5 * edge + rng.uniform(-0.02, 0.02, (6, 3)) * edge       # every sphere well inside the cell (10, 10, 10)
    few[:, 34:38] = ov.unit_quaternions(rng, 6)
    for bodies, sid in ((one, sid1), (few, sid6)):
        centre = bodies[:, 31:34] + bodies[:, 28:31]
        at = centre[rng.integers(0, len(bodies), 40)] + unit(rng.normal(size=(40, 3))) * rng.uniform(0.0, 4.0, (40, 1))
        q = capi.distances(at, ov.unit_quaternions(rng, 40), np.where(np.arange(40) % 4 == 0, POINT, 0), max_distance=rng.choice([0.25, 1.0, 2.0, np.inf], 40))
        with world_of(bodies, sid, polys) as w:
            hits = check_three_ways(w, dm.Scene(bodies, sid, polys), q)
        found = hits["body"] != capi.NO_HIT
        assert 10 < np.sum(found) and np.sum(~found) > 2


def test_bodies_around_the_origin_and_in_the_negative_octant():
    """Cell coordinates of either sign: bodies whose spheres contain the origin are binned in the cells -1 .. 0 on all three axes,
    others lie wholly at negative coordinates.  Queries from a few cells away with reaches several cells wide."""
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(411)
    n = 96
    bodies, sid = capi.scene_generate(KIND, 4, n)
    bodies[:, 34:38] = ov.unit_quaternions(rng, n)
    bodies[:, 31:34] = rng.uniform(-6.0, 2.0, (n, 3))
    bodies[:8, 31:34] = rng.uniform(-0.2, 0.2, (8, 3))               # around the origin
    bodies[:8, 31:34] -= np.array([capi.rigid_frame(row)[:3] - row[31:34] for row in bodies[:8]])   # (the frame's origin, not `position`)
    bodies[:8, 31:34] -= np.array([np.asarray(rm.rotate(tuple(bodies[i, 34:38]), tuple(float(x) for x in polys[int(sid[i])]["centroid"]))) for i in range(8)])
    groups = np.where(np.arange(n) < 8, 1, 2).astype(np.uint32)
    scene = dm.Scene(bodies, sid, polys, groups)
    edge = ov.cell_edge(polys, sid)
    cells_lo = np.floor((scene.centres - scene.body_radius[:, None]) / edge)
    cells_hi = np.floor((scene.centres + scene.body_radius[:, None]) / edge)
    assert ((cells_lo == -1) & (cells_hi == 0)).all(axis=1)[:8].all() and (cells_hi < 0).all(axis=1).sum() > 10
    m = 96
    at = scene.centres[rng.integers(0, 8, m)] + unit(rng.normal(size=(m, 3))) * rng.uniform(0.5, 3.0, (m, 1)) * edge
    aimed = capi.distances(at, ov.unit_quaternions(rng, m), np.where(np.arange(m) % 3 == 0, POINT, rng.integers(0, len(polys), m)),
                           max_distance=rng.choice([1.5, 2.5, 3.5], m) * edge, mask=1)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    with world_of(bodies, sid, polys) as w:
        w.set_collision_filters(filters)
        hits = check_three_ways(w, scene, aimed, MASKED)             # only the bodies around the origin answer
        assert np.sum(hits["body"] < 8) > 60 and (hits["body"][hits["body"] != capi.NO_HIT] < 8).all()
        hits = check_three_ways(w, scene, aimed)
        assert np.sum(hits["body"] >= 8) > 10
        q, _ = distance_families(rng, bodies, sid, polys, 192)
        hits = check_three_ways(w, scene, q)
        assert np.sum(hits["body"] != capi.NO_HIT) > 60


def test_ignore_body_and_masks():
    bodies, sid = ov.pile(1024)
    polys = capi.scene_polytopes(KIND)
    n = len(bodies)
    groups = (1 << (np.arange(n) % 3)).astype(np.uint32)
    groups[5::7] = 0                                                # bodies of no group answer unmasked queries only
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = groups, 0xFFFFFFFF
    rng = np.random.default_rng(381)
    with ov.stepped(bodies, sid, polys, 1, 10) as w:
        state = w.download()
        base, bad = distance_families(rng, state, sid, polys, 128)
        unfiltered = dm.Scene(state, sid, polys)
        q = base.copy()
        q["mask"] = 4
        got = check_three_ways(w, unfiltered, q, MASKED)             # no filters set: every body is in group ~0
        assert same_hits(got, unfiltered.distance(q))
        w.set_collision_filters(filters)
        scene = dm.Scene(state, sid, polys, groups)
        plain = check_three_ways(w, scene, base)
        found = plain["body"] != capi.NO_HIT
        assert np.any(groups[plain["body"][found]] == 0)
        # the winner of every query, ignored: the next body answers, further away or as far with a larger index
        again = base.copy()
        again["ignore_body"] = plain["body"]
        second = check_three_ways(w, scene, again)
        assert (second["body"][found] != plain["body"][found]).all()
        free = found & (base["ignore_body"] == capi.NO_HIT)          # (a query that ignored somebody else lets that body back in)
        assert free.sum() > 30 and (second["distance"][free] >= plain["distance"][free]).all()
        for mask in (1, 2, 4, 3, 0):
            q = base.copy()
            q["mask"] = mask
            hits = check_three_ways(w, scene, q, MASKED)
            got = hits["body"] != capi.NO_HIT
            assert np.all(groups[hits["body"][got]] & mask) and (mask == 0) == (not got.any())
            assert same_hits(w.distance(q), plain)                  # without the flag the mask field is ignored


def test_eight_and_nine_queries():
    """Either side of XPBD_DISTANCE_BRUTE_FORCE_QUERIES: eight queries take the brute-force path whatever the flags, nine the grid."""
    assert capi.DISTANCE_BRUTE_FORCE_QUERIES == 8
    bodies, sid = ov.pile(600)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(391)
    with world_of(bodies, sid, polys) as w:
        q, _ = distance_families(rng, bodies, sid, polys, 64)
        q = np.concatenate([q[:5], q[8:12]])                        # volumes and points inside the pile
        scene = dm.Scene(bodies, sid, polys)
        nine = check_three_ways(w, scene, q)
        eight = check_three_ways(w, scene, q[:8])
        assert same_hits(eight, nine[:8]) and (nine["body"] != capi.NO_HIT).sum() >= 4
        assert same_hits(w.distance(q[:1]), nine[:1]) and len(w.distance(q[:0])) == 0


def test_the_device_variant_equals_the_host_variant():
    """In a fresh child process that imports torch first (the library then binds to the HIP runtime torch carries)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "distance_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"grid": True, "brute": True, "few": True, "guard": True, "hits": True}


def test_all_four_queries_share_scratch_that_grows_under_use():
    """One world answers a ray cast, an overlap, a sweep and a distance query in turn, batches growing, then shrinking again: every
    call finds scratch and staging that another kind sized, and grows or reuses it.  Each answer equals, bit for bit, that of the
    same call on a fresh world with the same bodies."""
    import test_gpu_sweep as sw
    n = 300
    bodies, sid = ov.pile(n)
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(383)
    centre = bodies[:, 31:34] + bodies[:, 28:31]
    r = capi.rays(centre[rng.integers(0, n, 400)] + [0.0, 0.0, 50.0], [[0.0, 0.0, -1.0]])
    q = ov.query_families(rng, bodies, sid, polys, 200)
    s, _ = sw.sweep_families(rng, bodies, sid, polys, 320)
    d, _ = distance_families(rng, bodies, sid, polys, 640)
    calls = [("distance", d[:8], 0), ("raycast", r[:8], 0), ("distance", d[:100], 0), ("overlap", q, 0), ("distance", d[:320], 0), ("sweep", s, 0),
             ("distance", d, 0), ("raycast", r, 0), ("distance", d, BRUTE), ("sweep", s[:40], 0), ("distance", d[:9], 0), ("distance", d[:8], 0)]

    def ask(w, kind, batch, flags):
        if kind == "overlap":
            offsets, hits = w.overlap(batch, flags)
            return np.concatenate([offsets.view(np.uint8), hits.view(np.uint8)]), len(hits)
        hits = getattr(w, kind)(batch, flags)
        return hits.view(np.uint8), int(np.sum(hits["body"] != capi.NO_HIT))

    with world_of(bodies, sid, polys) as w:
        got = [ask(w, *call) for call in calls]
    for call, (answer, found) in zip(calls, got):
        with world_of(bodies, sid, polys) as fresh:
            want = ask(fresh, *call)
        assert found >= 4 and ov.same_bits(answer, want[0]), call[0]


def test_a_distance_query_has_no_side_effects():
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
                q, _ = distance_families(rng, bodies, sid, polys, 96)
                w.distance(q)
                w.distance(q[:4], BRUTE)
        results.append((w.download(), w.contacts(), w.contact_masks(10), np.array(w.contact_stats(), dtype=np.uint64),
                        np.array(w.contact_report_counts(), dtype=np.uint64)))
        w.close()
    for a, b in zip(*results):
        assert ov.same_bits(np.asarray(a), np.asarray(b))
    assert results[0][4][0] > 0


def test_distance_and_overlap_queries_agree_about_what_touches():
    """Where the overlap query lists bodies for a volume, the distance hit is XPBD_DISTANCE_OVERLAP with the first body of that
    segment; where it lists none, the feature is not OVERLAP."""
    bodies, sid = ov.pile()
    polys = capi.scene_polytopes(KIND)
    rng = np.random.default_rng(401)
    with ov.stepped(bodies, sid, polys, 1, 10) as w:
        state = w.download()
        centre = state[:, 31:34] + state[:, 28:31]
        n = 256
        pick = rng.integers(0, len(state), n)
        pos = centre[pick] + rng.normal(size=(n, 3)) * 0.7
        rot, shape = ov.unit_quaternions(rng, n), rng.integers(0, len(polys), n)
        ignore = np.where(np.arange(n) % 3 == 0, pick, capi.NO_HIT)
        offsets, listed = w.overlap(capi.overlap_queries(pos, rot, shape, ignore=ignore))
        hits = w.distance(capi.distances(pos, rot, shape, max_distance=rng.uniform(0.0, 2.0, n), ignore=ignore))
        counts = np.diff(offsets.astype(np.int64))
        assert np.sum(counts > 0) > 60 and np.sum(counts == 0) > 20
        touching = (hits["body"] != capi.NO_HIT) & (hits["feature"] == capi.DISTANCE_OVERLAP)
        assert (touching == (counts > 0)).all()
        first = listed["body"][offsets[:-1][counts > 0]]
        assert (hits["body"][counts > 0] == first).all() and not hits["distance"][counts > 0].any()


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
        q, _ = distance_families(np.random.default_rng(320 + n_ranks), state, sid, polys, 256)
        want = single.distance(q)
        assert np.sum(want["body"] != capi.NO_HIT) > 100 and np.any(q["ignore_body"] != capi.NO_HIT)
        assert same_hits(mw.distance(q), want)
        assert same_hits(mw.distance(q, BRUTE), want)
        assert same_hits(mw.distance(q[32:35]), single.distance(q[32:35]))
        single.set_collision_filters(filters)
        mw.set_collision_filters(filters)
        q["mask"] = np.random.default_rng(3).integers(0, 8, len(q))
        masked = single.distance(q, MASKED)
        assert not same_hits(masked, want) and same_hits(mw.distance(q, MASKED), masked)
    single.close()


def raw_distance(w, q, fn=None, flags=0, hits=True, queries=True):
    """One call of the C entry point: (rc, hits) with guard values in everything it may not touch."""
    fn = fn or capi.hip_lib().xpbd_world_distance
    out = np.zeros(len(q) + 2, dtype=capi.DISTANCE_HIT_DTYPE)
    out["body"] = 0xCDCDCDCD
    rc = fn(w._h, q.ctypes.data if queries else None, len(q), flags, out.ctypes.data if hits else None)
    return rc, out


def test_argument_errors_leave_the_outputs_untouched():
    bodies, sid = ov.pile(64)
    polys = capi.scene_polytopes(KIND)
    L = capi.hip_lib()
    q = capi.distances(bodies[:2, 31:34] + [0.0, 0.0, 3.0], [IDENT], [0, POINT])

    def untouched(rc, out):
        return rc == capi.E_INVALID and (out["body"] == 0xCDCDCDCD).all() and not out["distance"].any()

    def cases(w, fn, who):
        rc, out = raw_distance(w, q, fn)
        assert rc == capi.OK and (out["body"][:2] != 0xCDCDCDCD).all() and (out["body"][2:] == 0xCDCDCDCD).all()
        for flags in (4, capi.QUERY_TERRAIN, capi.QUERY_TERRAIN | BRUTE):
            assert untouched(*raw_distance(w, q, fn, flags=flags)) and b"unknown flags" in L.xpbd_last_error() and who in L.xpbd_last_error()
        assert untouched(*raw_distance(w, q, fn, queries=False)) and who in L.xpbd_last_error()
        assert raw_distance(w, q, fn, hits=False)[0] == capi.E_INVALID
        bad = q.copy()
        bad["reserved"][1] = 1
        assert untouched(*raw_distance(w, bad, fn)) and b"reserved" in L.xpbd_last_error() and who in L.xpbd_last_error()
        bad = q.copy()
        bad["shape"][0] = len(polys)                                 # no error: that query finds nothing
        rc, out = raw_distance(w, bad, fn)
        assert rc == capi.OK and out["body"][0] == capi.NO_HIT and out["body"][1] != capi.NO_HIT
        assert fn(w._h, None, 0, 0, None) == capi.OK                 # n_queries = 0

    with capi.World(mode=capi.MODE_CONTACTS) as w:
        assert untouched(*raw_distance(w, q)) and b"set_polytopes" in L.xpbd_last_error()     # no polytopes
        w.set_polytopes(polys)
        assert untouched(*raw_distance(w, q)) and b"no bodies" in L.xpbd_last_error() and b"xpbd_world_distance" in L.xpbd_last_error()
        w.upload(bodies, sid)
        cases(w, L.xpbd_world_distance, b"xpbd_world_distance")
        dev = L.xpbd_world_distance_device                          # (its checks run before it touches any pointer)
        assert dev(w._h, None, 2, 0, None) == capi.E_INVALID and dev(w._h, None, 0, 8, None) == capi.E_INVALID
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL) as mw:
        fn = L.xpbd_multi_world_distance
        assert untouched(*raw_distance(mw, q, fn)) and b"set_polytopes" in L.xpbd_last_error()
        mw.set_polytopes(polys)
        assert untouched(*raw_distance(mw, q, fn)) and b"no bodies" in L.xpbd_last_error()
        mw.upload(bodies, sid, 0, len(bodies))
        cases(mw, fn, b"xpbd_multi_world_distance")
