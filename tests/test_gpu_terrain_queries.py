"""The terrain in the scene queries (XPBD_QUERY_TERRAIN) on the GPU, bit for bit against the model of the definition
(tests/terrain_query_model.py) and the models of the bodies' answers: crafted and random rays against the terrain alone (walk ==
brute force == model), long walks, bodies and terrain together, sweeps, overlaps, the errors, no side effects, and the device
variants from a child process."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import overlap_model as om
import raycast_model as rm
import sweep_model as sm
import terrain_model as tm
import terrain_query_model as tq
from constraint_solver_amd import capi
from halo_common import pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
INF = np.inf
T, BRUTE = capi.QUERY_TERRAIN, 1                # (the brute-force bit is 1 in every family)
IDENT = [1.0, 0.0, 0.0, 0.0]
BOXES, MIXED = capi.SCENE_BOXES_DROP, capi.SCENE_MIXED_DROP
BINARY_ORIGIN, BINARY_CELL = (-1.0, 2.0), (0.5, 0.25)
PILE_TERRAIN = (tm.bumpy_field(9, 7, 11), (-8.0, -1.5), (1.3, 1.1))     # test_gpu_terrain.py's field under its 96-box pile


def same(a, b):
    return a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b) and a.tobytes() == b.tobytes()


def first_difference(a, b):
    for k in range(min(len(a), len(b))):
        if a[k:k + 1].tobytes() != b[k:k + 1].tobytes():
            return "record %d: %s != %s" % (k, a[k], b[k])
    return "lengths %d, %d" % (len(a), len(b))


def world(terrain, kind=BOXES, bodies=None, sid=None):
    w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=True)
    w.set_polytopes(capi.scene_polytopes(kind))
    if bodies is not None:
        w.upload(bodies, sid)
    if terrain is not None:
        w.set_terrain(*terrain)
    return w


def walk_brute_model(w, field, rays):
    """The terrain alone: the walk, brute force and the model agree in every field of every hit; the model's records."""
    want = tq.ray_hits(field, rays)
    walk, brute = w.raycast(rays, T), w.raycast(rays, T | BRUTE)
    assert same(walk, brute), first_difference(walk, brute)
    assert same(walk, want), first_difference(walk, want)
    return want


# ---- 1. crafted rays ----------------------------------------------------------------------------------------------------------
def crafted_rays(field):
    x0, y0, dx, dy, nx, ny = field.x0, field.y0, field.dx, field.dy, field.nx, field.ny
    xs, ys = [x0 + i * dx for i in range(nx)], [y0 + j * dy for j in range(ny)]
    out = []                                                    # (origin, direction, max_distance)
    for x in xs:
        for y in ys:
            for a, b in ((1.0, 1.0), (1.0, -1.0), (1.0, 0.5), (-0.5, 1.0), (-1.0, -1.0)):       # through every corner, at t = 1
                out.append(((x - a * dx, y - b * dy, 1.5), (a * dx, b * dy, -1.5), INF))
            out += [((x, y, 3.0), (0.0, 0.0, -1.0), INF), ((x, y, -3.0), (0.0, 0.0, 1.0), INF)]     # vertical, on corners
            out += [((x, y, -3.0), (0.25, -0.5, 0.125), INF), ((x, y, -3.0), (0.0, 0.0, -1.0), 2.0)]  # from under ground
    for j, y in enumerate(ys):                                  # along every grid line y = yj: above, descending, and under ground
        out += [((x0 - dx, y, 1.0), (1.0, 0.0, -0.125), INF), ((xs[-1] + dx, y, 1.0), (-1.0, 0.0, -0.125), INF), ((x0 - dx, y, -2.0), (1.0, 0.0, 0.0), INF)]
    for i, x in enumerate(xs):
        out += [((x, y0 - dy, 1.0), (0.0, 1.0, -0.125), INF), ((x, ys[-1] + dy, 1.0), (0.0, -1.0, -0.125), INF), ((x, ys[-1] + dy, -2.0), (0.0, -1.0, 0.0), INF)]
    for i in range(nx - 1):
        for j in range(ny - 1):
            x, y = xs[i], ys[j]
            out += [((x - dx, y - dy, 1.5), (dx, dy, -0.25), INF), ((x + 2 * dx, y + 2 * dy, 1.5), (-dx, -dy, -0.25), INF),   # along the diagonal
                    ((x - dx, y - dy, -2.0), (dx, dy, 0.0), INF), ((x + dx, y - dy, 1.5), (-dx, dy, -0.25), INF)]            # ... under ground; across
            out += [((x + 0.5 * dx, y, 3.0), (0.0, 0.0, -1.0), INF), ((x, y + 0.5 * dy, 3.0), (0.0, 0.0, -1.0), INF),        # vertical, on edges
                    ((x + 0.5 * dx, y + 0.5 * dy, 3.0), (0.0, 0.0, -1.0), INF), ((x + 0.75 * dx, y + 0.25 * dy, 3.0), (0.0, 0.0, -1.0), INF),
                    ((x + 0.25 * dx, y + 0.75 * dy, 3.0), (0.0, 0.0, -1.0), INF), ((x + 0.25 * dx, y + 0.75 * dy, -3.0), (0.0, 0.0, 1.0), INF)]
    mid_x, mid_y = x0 + 0.375 * dx, y0 + 0.625 * dy
    for o, d in (((x0 - 1.0, mid_y, -3.0), (1.0, 0.0, 0.0)), ((xs[-1] + 1.0, mid_y, -3.0), (-1.0, 0.0, 0.0)), ((mid_x, y0 - 1.0, -3.0), (0.0, 1.0, 0.0)),
                 ((mid_x, ys[-1] + 1.0, -3.0), (0.0, -2.0, 0.0)), ((x0 - 1.0, y0 - 1.0, -3.0), (1.0, 1.0, 0.125))):
        out.append((o, d, INF))                                 # from outside through the outer wall, below the surface
    out += [((mid_x, mid_y, 3.0), (0.0, 0.0, 1.0), INF), ((mid_x, mid_y, 3.0), (0.25, 0.5, 1.0), INF)]                       # above, pointing up
    out += [((x0 - 1.0, mid_y, 3.0), (0.0, 0.0, -1.0), INF), ((mid_x, ys[-1] + 0.5, 3.0), (0.0, 0.0, -1.0), INF),            # beside the field
            ((x0 - 1.0, mid_y, 3.0), (-1.0, 0.0, -1.0), INF), ((x0 - 1.0, y0 - 1.0, 0.0), (1.0, -1.0, 0.0), INF)]
    far = 2.0 ** 60
    out += [((-far, mid_y, -3.0), (1.0, 0.0, 0.0), INF), ((mid_x, far, -3.0), (0.0, -1.0, 0.0), INF), ((mid_x, mid_y, far), (0.0, 0.0, -1.0), INF),
            ((-far, -far * dy / dx + 0.0, -3.0), (dx, dy, 0.0), INF), ((far, mid_y, far), (-1.0, 0.0, -1.0), INF)]            # origins 2^60 away
    nan = math.nan
    out += [((nan, mid_y, 3.0), (0.0, 0.0, -1.0), INF), ((mid_x, mid_y, 3.0), (0.0, nan, -1.0), INF), ((mid_x, INF, 3.0), (0.0, 0.0, -1.0), INF),
            ((mid_x, mid_y, 3.0), (0.0, 0.0, -INF), INF), ((mid_x, mid_y, 3.0), (0.0, 0.0, 0.0), INF), ((mid_x, mid_y, -3.0), (0.0, -0.0, 0.0), INF),
            ((mid_x, mid_y, 3.0), (0.0, 0.0, -1.0), -1.0), ((mid_x, mid_y, 3.0), (0.0, 0.0, -1.0), nan)]                      # rays that hit nothing
    # direction components so small that a border's t overflows to +inf (finite and not zero: valid rays), in x, in y and in both,
    # max_distance +inf: hitting from above, missing upwards, and from under ground.  (tests/test_terrain_walk_host.py runs these
    # and the ones whose answer lies at t = +inf through a CPU build of the walk first.)
    for e in (5e-324, 1e-320, 1e-306):
        for s in (1.0, -1.0):
            out += [((mid_x, mid_y, 3.0), (s * e, 0.0, -1.0), INF), ((mid_x, mid_y, 3.0), (0.0, s * e, -1.0), INF),
                    ((mid_x, mid_y, 3.0), (s * e, -s * e, -1.0), INF), ((mid_x, mid_y, 3.0), (s * e, 0.125, -1.0), INF),
                    ((xs[0], ys[-1], 3.0), (s * e, s * e, -0.5), INF), ((mid_x, mid_y, 3.0), (s * e, s * e, 1.0), INF),
                    ((mid_x, mid_y, 3.0), (s * e, 0.0, 2.0), INF), ((mid_x, mid_y, -3.0), (s * e, s * e, 0.0), INF)]
    # max_distance exactly at the hit distance, and one ulp short of it
    for o, d in (((mid_x, mid_y, 3.0), (0.0, 0.0, -1.0)), ((x0 - dx, mid_y, 3.0), (1.0, 0.0, -4.0)), ((x0 - 1.0, mid_y, -3.0), (1.0, 0.0, 0.0))):
        hit = tq.raycast(field, o, d, INF)
        assert hit is not None and hit[0] > 0.0
        out += [(o, d, hit[0]), (o, d, float(np.nextafter(hit[0], 0.0)))]
    return capi.rays([o for o, _, _ in out], [d for _, d, _ in out], [m for _, _, m in out])


@pytest.mark.parametrize("heights", [np.array([[0.25, -0.5], [1.0, 0.125]]), tm.bumpy_field(4, 3, 7)], ids=["one_cell", "4x3"])
def test_crafted_rays_equal_the_model_bit_for_bit(heights):
    field = tm.Terrain(heights, BINARY_ORIGIN, BINARY_CELL)
    rays = crafted_rays(field)
    with world((heights, BINARY_ORIGIN, BINARY_CELL)) as w:
        want = walk_brute_model(w, field, rays)
        few = w.raycast(rays[:5], T)                            # (few rays: the bodies' pass is brute force, the terrain's the walk)
    assert same(few, want[:5])
    hit = want["body"] == capi.HIT_TERRAIN
    inside = hit & (want["face"] == capi.RAY_INSIDE)
    print("%d rays: %d hits, %d of them from inside, %d misses" % (len(rays), hit.sum(), inside.sum(), (~hit).sum()))
    assert len(rays) >= 9 and hit.sum() > 40 and inside.sum() >= 8 and (~hit).sum() >= 14
    assert (want["distance"][inside] == 0.0).all() and not want["normal"][inside].any()
    assert want["body"][-1] == capi.NO_HIT and want["body"][-2] == capi.HIT_TERRAIN              # one ulp short of it, exactly at it
    assert set(np.unique(want["body"])) == {capi.HIT_TERRAIN, capi.NO_HIT}
    tiny = ((np.abs(rays["direction"]) > 0.0) & (np.abs(rays["direction"]) < 1e-300)).any(axis=1)
    assert tiny.sum() == 48 and (want["body"][tiny] == capi.HIT_TERRAIN).sum() >= 24 and (want["body"][tiny] == capi.NO_HIT).sum() >= 12
    assert np.isfinite(want["distance"][hit]).all() and np.isfinite(want["point"]).all()


# ---- 2. random rays -----------------------------------------------------------------------------------------------------------
def test_random_rays_equal_the_model_bit_for_bit():
    heights = tq.recipe_heights()
    field = tm.Terrain(heights, tq.RECIPE_ORIGIN, tq.RECIPE_CELL)
    rays = capi.rays(*tq.random_rays(6000, 1))
    want = tq.ray_hits(field, rays)
    census = tq.classify(field, rays, want)
    print("top %d, wall or diagonal %d, inside %d, miss %d" % census)
    assert min(census) >= 0.03 * len(rays)                      # (the model's figures, before the device is asked)
    with world((heights, tq.RECIPE_ORIGIN, tq.RECIPE_CELL)) as w:
        walk, brute = w.raycast(rays, T), w.raycast(rays, T | BRUTE)
    assert same(walk, brute), first_difference(walk, brute)
    assert same(walk, want), first_difference(walk, want)


# ---- 3. long walks ------------------------------------------------------------------------------------------------------------
def test_long_grazing_walks_equal_brute_force():
    n, cell = 65, 0.25
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    heights = 0.15 * np.sin(0.35 * i + 0.2) * np.cos(0.27 * j)
    origin = (-8.0, -8.0)
    rng = np.random.default_rng(9)
    k = 2048
    angle = rng.uniform(0.0, 2.0 * np.pi, k)
    d = np.stack([np.cos(angle), np.sin(angle), -rng.uniform(0.02, 0.08, k)], axis=1)
    d[::16, 0], d[1::16, 1] = 0.0, 0.0                          # some along the axes ...
    d[2::16, :2] = [[cell, cell]]                               # ... and along the diagonals
    o = np.stack([rng.uniform(-7.0, 7.0, k), rng.uniform(-7.0, 7.0, k), rng.uniform(0.16, 0.4, k)], axis=1)
    o[4::16, :2] -= 12.0 * d[4::16, :2]                         # from outside the field
    o[3::16, :2] = np.round(o[3::16, :2] / cell) * cell         # from corners
    rays = capi.rays(o, d, np.where(np.arange(k) % 5 == 0, 12.0, INF))
    with world((heights, origin, (cell, cell))) as w:
        walk, brute = w.raycast(rays, T), w.raycast(rays, T | BRUTE)
    assert same(walk, brute), first_difference(walk, brute)
    hit = walk["body"] == capi.HIT_TERRAIN
    run = walk["distance"][hit] * np.linalg.norm(d[hit, :2], axis=1) / cell
    print("%d of %d rays hit; cells crossed before the hit: median %.0f, max %.0f" % (hit.sum(), k, np.median(run), run.max()))
    assert hit.sum() > k // 4 and np.median(run) >= 10.0 and (walk["face"][hit] != capi.RAY_INSIDE).sum() > k // 5


# ---- 4. bodies and terrain together ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def settled_pile():
    """The 96-box pile of test_gpu_terrain.py settled on its 9 x 7 field: (state, shape ids)."""
    bodies, sid = pile(capi, BOXES, 96, 3, 4.0, 3.0)
    with world(PILE_TERRAIN, BOXES, bodies, sid) as w:
        w.set_max_depenetration_speed(3.0)
        for _ in range(40):
            w.step(DT, 6)
        state = w.download()
    assert not np.isnan(state).any()
    return state, sid


def pile_rays(k, seed):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-9.0, 7.0, k), rng.uniform(-3.0, 7.0, k), rng.uniform(1.5, 6.0, k)], axis=1)
    d = rng.normal(size=(k, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 0.3
    return capi.rays(o, d, np.where(np.arange(k) % 3 == 0, 6.0, INF), ignore=np.where(np.arange(k) % 7 == 0, np.arange(k) % 96, capi.NO_HIT))


def test_bodies_and_terrain_together_equal_the_models(settled_pile):
    state, sid = settled_pile
    polys = capi.scene_polytopes(BOXES)
    field = tm.Terrain(*PILE_TERRAIN)
    rays = pile_rays(4096, 21)
    of_bodies = tq.body_ray_hits(rm.raycast(state, sid, polys, rays)[0])
    want = tq.merge_ray_hits(of_bodies, tq.ray_hits(field, rays))
    on_terrain, missed = want["body"] == capi.HIT_TERRAIN, want["body"] == capi.NO_HIT
    print("%d terrain hits, %d body hits, %d misses" % (on_terrain.sum(), (~on_terrain & ~missed).sum(), missed.sum()))
    assert min(on_terrain.sum(), (~on_terrain & ~missed).sum(), missed.sum()) >= 0.1 * len(rays)
    groups = np.zeros(len(state), dtype=capi.COLLISION_FILTER_DTYPE)
    groups["group"], groups["mask"] = 1 << (np.arange(len(state)) % 3), 0xFFFFFFFF
    q = capi.overlap_queries(state[:40, 31:34] + state[:40, 28:31], [IDENT], 0)
    s = capi.sweeps(state[:40, 31:34] + [0.0, 0.0, 4.0], [IDENT], [0.0, 0.0, -1.0], 0)
    with world(PILE_TERRAIN, BOXES, state, sid) as w:
        w.set_collision_filters(groups)
        grid, brute = w.raycast(rays, T), w.raycast(rays, T | BRUTE)
        assert same(grid, brute), first_difference(grid, brute)
        assert same(grid, want), first_difference(grid, want)
        masked = w.raycast(rays, T, mask=2)                     # the mask does not concern the terrain
        assert (masked["body"] == capi.HIT_TERRAIN).sum() > on_terrain.sum() and not same(masked, grid)
        # without the flag a world with a terrain answers as one without
        qm, sm_ = q.copy(), s.copy()
        qm["mask"], sm_["mask"] = 2, 2

        def records():                                          # every existing host form with one result per record
            return [w.raycast(rays), w.raycast(rays, BRUTE), w.raycast(rays, mask=2), w.raycast(rays, BRUTE, mask=2), w.raycast(rays[:5]),
                    w.sweep(s), w.sweep(s, BRUTE), w.sweep(sm_, capi.SWEEP_MASKED), w.sweep(sm_, capi.SWEEP_MASKED | BRUTE), w.sweep(s[:5])]

        def lists():
            return [w.overlap(q), w.overlap(q, BRUTE), w.overlap(qm, capi.OVERLAP_MASKED), w.overlap(qm, capi.OVERLAP_MASKED | BRUTE)]

        plain, plain_overlap = records(), lists()
        assert same(plain[0], of_bodies) and not same(plain[7], plain[5]) and len(plain_overlap[2][1]) < len(plain_overlap[0][1])
        w.set_terrain(None)
        for a, b in zip(plain, records()):
            assert same(a, b)
        for a, b in zip(plain_overlap, lists()):
            assert np.array_equal(a[0], b[0]) and same(a[1], b[1]) and len(a[1]) > 0


# ---- 5. sweeps -----------------------------------------------------------------------------------------------------------------
def unit_quaternions(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def terrain_sweeps(rng, k, n_shapes):
    """Volumes of every shape over and around PILE_TERRAIN's field and the pile, swept down, sideways and up; some start under
    ground, some beside the field, some cannot hit anything."""
    pos = np.stack([rng.uniform(-8.5, 4.5, k), rng.uniform(-2.0, 5.5, k), rng.uniform(0.8, 5.0, k)], axis=1)
    d = rng.normal(size=(k, 3)) * [1.0, 1.0, 0.3]
    d[:, 2] -= 0.6
    d[::4] = [0.0, 0.0, -1.0]                                   # straight down
    d[1::8, 2] = 0.0                                            # sideways
    pos[1::8, 2] = rng.uniform(-0.3, 0.9, len(pos[1::8]))
    pos[2::16, 2] = rng.uniform(-2.0, -0.7, len(pos[2::16]))    # starts under ground
    rot = unit_quaternions(rng, k)
    rot[::3] = IDENT
    q = capi.sweeps(pos, rot, d, rng.integers(0, n_shapes, k), max_distance=np.where(np.arange(k) % 5 == 0, 2.5, INF))
    q["direction"][5::64] = 0.0
    q["shape"][6::64] = n_shapes
    q["max_distance"][7::64] = np.nan
    q["position"][8::64, 1] = np.inf
    return q


@pytest.mark.parametrize("with_pile", [False, True])
def test_sweeps_equal_the_models(with_pile):
    polys = capi.scene_polytopes(MIXED)
    field = tm.Terrain(*PILE_TERRAIN)
    bodies, sid = pile(capi, MIXED, 120 if with_pile else 1, 5, 4.0, 3.0)
    if not with_pile:
        bodies[:, 31:34] = [300.0, 300.0, 300.0]               # (a sweep needs a resident body: this one is out of everybody's way)
    q = terrain_sweeps(np.random.default_rng(31 + with_pile), 384, len(polys))
    of_bodies = sm.Scene(bodies, sid, polys).sweep(q)
    want = tq.sweep_hits(field, polys, q, of_bodies)
    on_terrain = want["body"] == capi.HIT_TERRAIN
    initial = on_terrain & (want["feature"] == capi.SWEEP_INITIAL)
    kept = (of_bodies["body"] != capi.NO_HIT) & (want["body"] == of_bodies["body"])
    print("%d sweeps: %d stop at the terrain (%d start in it), %d keep their body, %d miss" %
          (len(q), on_terrain.sum(), initial.sum(), kept.sum(), (want["body"] == capi.NO_HIT).sum()))
    assert (on_terrain & ~initial).sum() > 50 and initial.sum() >= 10 and (want["body"] == capi.NO_HIT).sum() >= 20
    assert len(np.unique(q["shape"][on_terrain])) == len(polys) > 1
    if with_pile:
        assert kept.sum() >= 20                                 # a sweep that a body stops first keeps the body's hit
    with world(PILE_TERRAIN, MIXED, bodies, sid) as w:
        grid, brute, few = w.sweep(q, T), w.sweep(q, T | BRUTE), w.sweep(q[:6], T)
        plain = w.sweep(q)
    assert same(grid, brute), first_difference(grid, brute)
    assert same(grid, want), first_difference(grid, want)
    assert same(few, want[:6]) and same(plain, of_bodies)
    assert same(grid[kept], of_bodies[kept])


def test_a_box_set_down_by_a_sweep_is_free_just_before_and_touches_just_after():
    polys = capi.scene_polytopes(BOXES)
    rng = np.random.default_rng(41)
    k = 64
    pos = np.stack([rng.uniform(-7.5, 1.5, k), rng.uniform(-1.0, 4.0, k), rng.uniform(2.0, 4.0, k)], axis=1)
    d = np.stack([rng.uniform(-0.2, 0.2, k), rng.uniform(-0.2, 0.2, k), -np.ones(k)], axis=1)
    rot = unit_quaternions(rng, k)
    far, far_sid = pile(capi, BOXES, 1, 5, 4.0, 3.0)
    far[:, 31:34] = [300.0, 300.0, 300.0]
    with world(PILE_TERRAIN, BOXES, far, far_sid) as w:
        hits = w.sweep(capi.sweeps(pos, rot, d, 0), T)
        landed = (hits["body"] == capi.HIT_TERRAIN) & (hits["feature"] == capi.FEATURE_FACE_B)
        assert landed.sum() > k // 2
        for shift, touching in ((-1e-9, False), (1e-9, True)):
            offsets, found = w.overlap(capi.overlap_queries(hits["position"][landed] + shift * d[landed], rot[landed], 0), T)
            counts = np.diff(offsets.astype(np.int64))
            assert (counts == (1 if touching else 0)).all()
            assert (found["body"] == capi.HIT_TERRAIN).all() and (found["separation"] < 0.0).all() and (found["separation"] > -1e-8).all()


# ---- 6. overlaps ---------------------------------------------------------------------------------------------------------------
def expected_overlap(field, polys, q, of_bodies):
    """The bodies' (offsets, hits) with the terrain's entry appended to every segment that has one."""
    offsets, hits = of_bodies
    out, new_offsets = [], [0]
    for k in range(len(q)):
        out += [hits[offsets[k]:offsets[k + 1]]]
        s = tq.overlap_entry(field, polys[int(q["shape"][k])], q["position"][k], q["rotation"][k]) if np.isfinite(q["position"][k]).all() else None
        if s is not None:
            entry = np.zeros(1, dtype=capi.OVERLAP_HIT_DTYPE)
            entry["body"], entry["feature"], entry["separation"] = capi.HIT_TERRAIN, capi.FEATURE_FACE_B, s
            out.append(entry)
        new_offsets.append(sum(len(x) for x in out))
    return np.array(new_offsets, dtype=np.uint32), np.concatenate(out) if out else hits[:0]


def overlap_volumes(rng, k):
    """Boxes at random poses around PILE_TERRAIN's field and the pile, half of them where the two meet, some beside the field."""
    pos = np.stack([rng.uniform(-9.5, 6.0, k), rng.uniform(-2.5, 6.5, k), rng.uniform(-0.8, 1.5, k)], axis=1)
    pos[::2] = np.stack([rng.uniform(-1.0, 3.0, k), rng.uniform(0.0, 4.0, k), rng.uniform(-0.3, 0.8, k)], axis=1)[::2]
    pos[5::32, 0], pos[5::32, 2] = -12.0, -0.7                  # (no box of the scene reaches 4 m)
    return pos, capi.overlap_queries(pos, unit_quaternions(rng, k), 0)


def test_overlaps_equal_the_models(settled_pile):
    state, sid = settled_pile
    polys = capi.scene_polytopes(BOXES)
    field = tm.Terrain(*PILE_TERRAIN)
    rng = np.random.default_rng(51)
    k = 256
    pos, q = overlap_volumes(rng, k)
    q["position"][7::64, 0] = np.nan
    want = expected_overlap(field, polys, q, om.Scene(state, sid, polys).overlap(q))
    counts = np.diff(want[0].astype(np.int64))
    with_terrain = np.array([(want[1]["body"][a:b] == capi.HIT_TERRAIN).any() for a, b in zip(want[0][:-1], want[0][1:])])
    both = with_terrain & (counts >= 2)
    print("%d queries: %d touch the terrain, %d of them bodies too, %d touch nothing" % (k, with_terrain.sum(), both.sum(), (counts == 0).sum()))
    assert with_terrain.sum() > 60 and both.sum() >= 10 and (counts == 0).sum() >= 20 and (~with_terrain & (counts > 0)).sum() >= 10
    outside = (pos[:, 0] < -11.0) & (pos[:, 2] < -0.5)           # a volume beside the field, however low, has no entry
    assert outside.sum() >= 3 and not with_terrain[outside].any()
    L = capi.hip_lib()
    with world(PILE_TERRAIN, BOXES, state, sid) as w:
        grid, brute = w.overlap(q, T), w.overlap(q, T | BRUTE)
        for got in (grid, brute):
            assert np.array_equal(got[0], want[0]) and same(got[1], want[1]), first_difference(got[1], want[1])
        for a, b in zip(want[0][:-1], want[0][1:]):             # the terrain's entry is the last of its segment
            assert (want[1]["body"][a:b - 1] != capi.HIT_TERRAIN).all()
        # a count-only call, and a cap that cuts the last terrain entry off
        total = want[0][-1]
        assert want[1]["body"][-1] == capi.HIT_TERRAIN
        for flags in (T, T | BRUTE):
            offsets, n_out = np.zeros(k + 1, dtype=np.uint32), capi.C.c_uint32(0)
            rc = L.xpbd_world_overlap(w._h, q.ctypes.data, k, flags, offsets.ctypes.data, None, 0, capi.C.byref(n_out))
            assert rc == capi.E_CAPACITY and n_out.value == total and np.array_equal(offsets, want[0])
            hits = np.zeros(total, dtype=capi.OVERLAP_HIT_DTYPE)
            hits["body"] = 0xCDCDCDCD
            rc = L.xpbd_world_overlap(w._h, q.ctypes.data, k, flags, offsets.ctypes.data, hits.ctypes.data, total - 1, capi.C.byref(n_out))
            assert rc == capi.E_CAPACITY and n_out.value == total and np.array_equal(offsets, want[0])
            assert same(hits[:total - 1], want[1][:total - 1]) and hits["body"][-1] == 0xCDCDCDCD
        plain = w.overlap(q)
        assert not (plain[1]["body"] == capi.HIT_TERRAIN).any() and len(plain[1]) == total - with_terrain.sum()


def integrated_at_rest(rot):
    """What Rigid::integrate makes of the rotation of a body without velocities and forces: q * (1 / sqrt(s s + (x x + y y + z z)))."""
    rot = np.array(rot, dtype=np.float64)
    m2 = rot[:, 0] * rot[:, 0] + (rot[:, 1] * rot[:, 1] + rot[:, 2] * rot[:, 2] + rot[:, 3] * rot[:, 3])
    return rot * (1.0 / np.sqrt(m2))[:, None]


def test_a_resident_body_touches_the_terrain_iff_the_stepper_gives_it_a_ground_contact(settled_pile):
    """The settled pile's bodies at rest (velocities and forces zeroed, so that the next substep's integrate leaves every position
    as it is and only normalises the rotation): the overlap query of every body's own shape at the frame of that pose lists the
    terrain iff that substep's ground contact mask of the body is nonzero."""
    state, sid = settled_pile
    rest = state.copy()
    rest[:, 10:28] = 0.0                                        # forces, torques, velocities
    rest[:, 33] -= 0.003                                        # (the solver has pushed the resting vertices out to s = 0 or just above)
    posed = rest.copy()
    posed[:, 34:38] = integrated_at_rest(rest[:, 34:38])
    frames = np.array([capi.rigid_frame(row) for row in posed])
    q = capi.overlap_queries(frames[:, :3], frames[:, 3:], sid, ignore=np.arange(len(rest)))
    with world(PILE_TERRAIN, BOXES, rest, sid) as w:
        offsets, hits = w.overlap(q, T)
        w.step(DT, 1)
        masks = w.contact_masks(1)[0]
    listed = np.array([(hits["body"][a:b] == capi.HIT_TERRAIN).any() for a, b in zip(offsets[:-1], offsets[1:])])
    print("%d of %d bodies touch the terrain" % (listed.sum(), len(rest)))
    assert 8 <= listed.sum() <= len(rest) - 8
    assert np.array_equal(listed, masks[:len(rest)] != 0)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_the_flag_needs_a_terrain_and_stays_unknown_where_there_is_none():
    bodies, sid = pile(capi, BOXES, 32, 3, 4.0, 3.0)
    polys = capi.scene_polytopes(BOXES)
    L = capi.hip_lib()
    rays = capi.rays(bodies[:12, 31:34] + [0.0, 0.0, 5.0], [[0.0, 0.0, -1.0]])
    q = capi.overlap_queries(bodies[:12, 31:34], [IDENT], 0)
    s = capi.sweeps(bodies[:12, 31:34] + [0.0, 0.0, 5.0], [IDENT], [0.0, 0.0, -1.0], 0)

    def calls(h, ray_fn, overlap_fn, sweep_fn, flags):
        """(rc, message, outputs untouched) of the three host calls with these flags."""
        out = []
        hits = np.zeros(14, dtype=capi.RAY_HIT_DTYPE)
        hits["body"] = 0xCDCDCDCD
        rc = ray_fn(h, rays.ctypes.data, 12, flags, hits.ctypes.data)
        out.append((rc, L.xpbd_last_error(), (hits["body"] == 0xCDCDCDCD).all() and not hits["distance"].any()))
        offsets, found, n_out = np.full(13, 0xCDCDCDCD, dtype=np.uint32), np.zeros(64, dtype=capi.OVERLAP_HIT_DTYPE), capi.C.c_uint32(77)
        found["body"] = 0xCDCDCDCD
        rc = overlap_fn(h, q.ctypes.data, 12, flags, offsets.ctypes.data, found.ctypes.data, 64, capi.C.byref(n_out))
        out.append((rc, L.xpbd_last_error(), (offsets == 0xCDCDCDCD).all() and (found["body"] == 0xCDCDCDCD).all() and n_out.value == 77))
        swept = np.zeros(14, dtype=capi.SWEEP_HIT_DTYPE)
        swept["body"] = 0xCDCDCDCD
        rc = sweep_fn(h, s.ctypes.data, 12, flags, swept.ctypes.data)
        out.append((rc, L.xpbd_last_error(), (swept["body"] == 0xCDCDCDCD).all() and not swept["distance"].any()))
        return out

    single = (L.xpbd_world_raycast, L.xpbd_world_overlap, L.xpbd_world_sweep)
    with world(None, BOXES, bodies, sid) as w:
        for rc, message, untouched in calls(w._h, *single, T) + calls(w._h, *single, T | BRUTE):
            assert rc == capi.E_INVALID and b"xpbd_world_set_terrain" in message and untouched        # the flag without a terrain
        hits = np.zeros(12, dtype=capi.RAY_HIT_DTYPE)
        assert L.xpbd_world_raycast_masked(w._h, rays.ctypes.data, 12, T, 1, hits.ctypes.data) == capi.E_INVALID
        for dev in (L.xpbd_world_raycast_device, L.xpbd_world_sweep_device):                          # (checked before any pointer is touched)
            assert dev(w._h, rays.ctypes.data, 12, T, hits.ctypes.data) == capi.E_INVALID and b"xpbd_world_set_terrain" in L.xpbd_last_error()
        w.set_terrain(*PILE_TERRAIN)
        assert all(rc in (capi.OK, capi.E_CAPACITY) for rc, _, _ in calls(w._h, *single, T))
        for flags, which in ((2, 0), (2 | T, 0), (4, 1), (4 | T, 1), (4, 2), (4 | T, 2), (0x200, 0), (0x80, 1), (0x200 | T, 2)):
            rc, message, untouched = calls(w._h, *single, flags)[which]
            assert rc == capi.E_INVALID and b"unknown flags" in message and untouched
        w.set_terrain(None)
        assert all(rc == capi.E_INVALID for rc, _, _ in calls(w._h, *single, T))
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL) as mw:
        mw.set_polytopes(polys)
        mw.upload(bodies, sid, 0, len(bodies))
        multi = (L.xpbd_multi_world_raycast, L.xpbd_multi_world_overlap, L.xpbd_multi_world_sweep)
        for rc, message, untouched in calls(mw._h, *multi, T):
            assert rc == capi.E_INVALID and b"unknown flags" in message and untouched
        assert all(rc in (capi.OK, capi.E_CAPACITY) for rc, _, _ in calls(mw._h, *multi, 0))


# ---- 8. no side effects ----------------------------------------------------------------------------------------------------------
def test_stepping_after_the_queries_gives_the_bits_of_stepping_without_them():
    bodies, sid = pile(capi, BOXES, 96, 3, 4.0, 3.0)
    rays = pile_rays(512, 5)
    spots = bodies[:64, 31:34] * [1.0, 1.0, 0.1]
    spots[::2] -= [5.0, 0.0, 0.4]                               # every other one beside the pile, over the field
    q = capi.overlap_queries(spots, [IDENT], 0)
    s = capi.sweeps(spots + [0.0, 0.0, 4.0], [IDENT], [0.0, 0.0, -1.0], 0)
    results = []
    for ask in (False, True):
        with world(PILE_TERRAIN, BOXES, bodies, sid) as w:
            w.set_contact_report(True)
            for _ in range(8):
                w.step(DT, 6)
                if ask:
                    found = (w.raycast(rays, T), w.overlap(q, T)[1], w.sweep(s, T))
                    assert all((x["body"] == capi.HIT_TERRAIN).any() for x in found)
                    few = [np.nonzero(x["body"] == capi.HIT_TERRAIN)[0][:4] for x in (found[0], found[2])]     # (few: the bodies' brute-force path)
                    assert same(w.raycast(rays[few[0]], T | BRUTE), found[0][few[0]]) and same(w.sweep(s[few[1]], T | BRUTE), found[2][few[1]])
            results.append((w.download(), w.contacts(), w.contact_masks(6), np.array(w.contact_stats(), dtype=np.uint64),
                            np.array(w.contact_report_counts(), dtype=np.uint64)))
    for a, b in zip(*results):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert results[0][2].any() and not np.isnan(results[0][0]).any()


# ---- 9. the device variants ------------------------------------------------------------------------------------------------------
def test_the_device_variants_equal_the_host_variants():
    """In a fresh child process that imports torch first (the library then binds to the HIP runtime torch carries)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "terrain_query_device_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res and all(res.values()), res
    assert set(res) >= {"rays", "rays_brute", "rays_masked", "rays_plain", "sweeps", "sweeps_brute", "sweeps_plain", "overlaps", "overlaps_brute",
                        "overlaps_plain", "overlaps_count_only", "guard", "terrain_seen", "rays_plain_no_terrain", "rays_masked_no_terrain",
                        "sweeps_plain_no_terrain", "overlaps_plain_no_terrain"}
