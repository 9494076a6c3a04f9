"""Heightfield terrain (xpbd_world_set_terrain, xpbd_world_sample_terrain) on the GPU: the lookup alone against the model
(tests/terrain_model.py), bit for bit; a flat field changes no value of a world on the plane; on a bumpy field that covers only
part of the scene the device equals the model bit for bit, through xpbd_world_step and the split API; restitution on a slope;
a box sticks and slides on a real slope by the project's thresholds; nothing tunnels; lifetime, errors, the headless driver."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import material_model as mm
import oracle_binding as ob
import terrain_model as tm
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, chain_joints, pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = 9.81
INF = np.inf
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
MUS = np.array([0.0, 0.2, 0.5, 1.0, INF])
PLANE = "no set_terrain call"


def world(kind, bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT, trace=False):
    w = capi.World(mode=mode, trace_contacts=trace)
    w.set_polytopes(capi.scene_polytopes(kind))
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


def advance(w, frames, substeps, split=False):
    for _ in range(frames):
        if split:
            w.contacts_begin(DT)
            for _ in range(substeps):
                w.contacts_substep(DT / substeps)
        else:
            w.step(DT, substeps)


def run(kind, bodies, sid, frames, substeps, terrain=PLANE, mu=None, ground_mu=INF, speed=0.0, e=None, ground_e=0.0, joints=None,
        narrowphase=capi.NARROWPHASE_SAT, mode=capi.MODE_CONTACTS, split=False, masks=False):
    """The final state; with masks=True also the contact masks of every substep and the contacts of the last one."""
    with world(kind, bodies, sid, mode, narrowphase, trace=masks) as w:
        if joints is not None:
            w.set_joints(joints)
        if speed:
            w.set_max_depenetration_speed(speed)
        if mu is not None:
            w.set_materials(mu, ground_mu)
        if e is not None:
            w.set_restitution(e, ground_e, 0.0)
        if terrain is not PLANE:
            w.set_terrain(*terrain)
        if not masks:
            advance(w, frames, substeps, split)
            return w.download()
        rows = []
        for _ in range(frames):
            w.step(DT, substeps)
            rows.append(w.contact_masks(substeps))
        return w.download(), np.concatenate(rows), w.contacts()


def with_far_field(bodies, sid, kind, count, seed):
    """test_gpu_materials.py's: the scene followed by `count` bodies on a 4 m grid 200 m away, so the scene keeps its indices."""
    far, far_sid = capi.scene_generate(kind, seed, count)
    k = np.arange(count)
    far[:, 31] = 200.0 + 4.0 * (k % 128)
    far[:, 32] = 4.0 * (k // 128)
    far[:, 22:25] *= 0.3
    return np.concatenate([bodies, far]), np.concatenate([sid, far_sid])


def same_values(a, b):
    """Bit for bit, a NaN equal to a NaN whatever its payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


# ---- 1. the lookup alone ---------------------------------------------------------------------------------------------------
def probe_points(nx, ny, origin, cell):
    x0, y0 = origin
    dx, dy = cell
    xs = [x0 + i * dx for i in range(nx)]
    ys = [y0 + j * dy for j in range(ny)]
    pts = [(x, y) for x in xs for y in ys]                                                  # cell corners (the far ones: outside)
    for i in range(nx - 1):
        for j in range(ny - 1):
            pts += [(xs[i] + t * dx, ys[j] + t * dy) for t in (0.25, 0.5, 0.75)]             # the diagonal: fu == fv
            pts += [(xs[i] + 0.5 * dx, ys[j]), (xs[i], ys[j] + 0.5 * dy)]                    # cell edges
            pts += [(xs[i] + a * dx, ys[j] + b * dy) for a, b in ((0.7, 0.2), (0.9, 0.4), (0.2, 0.7), (0.4, 0.9))]  # both triangles
    far_x, far_y = xs[-1], ys[-1]
    before_x, before_y = float(np.nextafter(far_x, -INF)), float(np.nextafter(far_y, -INF))
    pts += [(before_x, ys[0]), (xs[0], before_y), (before_x, before_y), (far_x, ys[0]), (xs[0], far_y), (far_x, far_y),
            (float(np.nextafter(far_x, INF)), ys[0])]                                        # the far edge: half-open
    pts += [(float(np.nextafter(x0, -INF)), ys[0]), (xs[0], float(np.nextafter(y0, -INF))), (x0 - 1.0, y0 - 1.0), (x0 - 1e-300, ys[0])]
    pts += [(math.nan, ys[0]), (xs[0], math.nan), (math.nan, math.nan)]
    pts += [(1e300, ys[0]), (-1e300, ys[0]), (xs[0], 1e300), (xs[0], -1e300), (1e300, 1e300), (-1e300, 1e300), (INF, ys[0]), (xs[0], -INF)]
    return np.array(pts)


# the 2 x 2 field has binary spacing, so that u, v and with them fu == fv are exact; the 4 x 3 one has odd spacing
@pytest.mark.parametrize("heights,origin,cell", [(np.array([[0.25, -0.5], [1.0, 0.125]]), (-1.0, 2.0), (0.5, 0.25)),
                                                 (tm.bumpy_field(4, 3, 7), (-1.3, 0.7), (0.7, 0.9))])
def test_sample_terrain_equals_the_model_bit_for_bit(heights, origin, cell):
    ny, nx = heights.shape
    field = tm.Terrain(heights, origin, cell)
    pts = probe_points(nx, ny, origin, cell)
    want = [field.sample(float(x), float(y)) for x, y in pts]
    want_h, want_n = np.array([h for h, _ in want]), np.array([n for _, n in want])
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        with pytest.raises(capi.XpbdError) as e:
            w.sample_terrain(pts)
        assert e.value.code == capi.E_INVALID                                                # no terrain yet
        w.set_terrain(heights, origin, cell)
        got_h, got_n = w.sample_terrain(pts)
        alone = w.sample_terrain(pts, normals=False)
        assert len(w.sample_terrain(np.zeros((0, 2)))[0]) == 0
    inside = ~np.isnan(want_h)
    print("%d points, %d inside" % (len(pts), inside.sum()))
    assert inside.sum() > 9 * (nx - 1) * (ny - 1) and (~inside).sum() >= 20
    assert same_values(got_h, want_h) and same_values(alone, want_h)
    assert np.array_equal(got_n.view(np.uint64), want_n.view(np.uint64))
    assert np.array_equal(got_n[~inside], np.zeros(((~inside).sum(), 3)))
    if cell == (0.5, 0.25):                                     # exact arithmetic: what is inside is known without the model
        x_far, y_far = origin[0] + cell[0], origin[1] + cell[1]
        expect = (pts[:, 0] >= origin[0]) & (pts[:, 0] < x_far) & (pts[:, 1] >= origin[1]) & (pts[:, 1] < y_far)
        assert np.array_equal(inside, expect)
        u, v = (pts[inside, 0] - origin[0]) / cell[0], (pts[inside, 1] - origin[1]) / cell[1]
        assert (u == v).sum() >= 4 and (u > v).sum() >= 4 and (u < v).sum() >= 4


# ---- 2. a flat field changes no value ---------------------------------------------------------------------------------------
FLAT_ORIGIN, FLAT_CELL = (-60.3, -50.9), (0.7, 0.9)


def flat_terrain(reach_x, reach_y):
    nx = int(math.ceil((reach_x - FLAT_ORIGIN[0]) / FLAT_CELL[0])) + 2
    ny = int(math.ceil((reach_y - FLAT_ORIGIN[1]) / FLAT_CELL[1])) + 2
    return tm.flat_field(nx, ny), FLAT_ORIGIN, FLAT_CELL


@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
@pytest.mark.parametrize("big", [False, True])
def test_flat_field_changes_no_value(narrowphase, big):
    """A pile of 160 boxes with ground and pair contacts and chain joints, alone (eight lanes per body) or in front of 16 400
    far-away bodies over the same field (one lane per body): poses, the masks of every substep and the contacts are equal.
    The world with the field runs the unfused schedule, the world without the fused one."""
    kind, n, frames, substeps = capi.SCENE_BOXES_DROP, 160, 12, 10
    bodies, sid = pile(capi, kind, n, 6, 4.0, 6.0)
    joints = chain_joints(capi, n)
    scene, scene_sid = with_far_field(bodies, sid, kind, SMALL_WORLD + 16, 9) if big else (bodies, sid)
    flat = flat_terrain(760.0, 560.0) if big else flat_terrain(60.0, 60.0)
    plain, plain_masks, plain_contacts = run(kind, scene, scene_sid, frames, substeps, joints=joints, narrowphase=narrowphase, masks=True)
    got, got_masks, got_contacts = run(kind, scene, scene_sid, frames, substeps, flat, joints=joints, narrowphase=narrowphase, masks=True)
    assert not np.isnan(plain).any() and plain_masks.any()
    assert plain[:, 31].min() > FLAT_ORIGIN[0] + 2.0 and plain[:, 32].min() > FLAT_ORIGIN[1] + 2.0     # (nobody left the field)
    assert plain[:, 31].max() < (760.0 if big else 60.0) and plain[:, 32].max() < (560.0 if big else 60.0)
    assert np.array_equal(got, plain)
    assert np.array_equal(got_masks, plain_masks) and np.array_equal(got_contacts, plain_contacts)


def test_clearing_a_bumpy_field_restores_the_plane_world():
    kind, n = capi.SCENE_BOXES_DROP, 96
    bodies, sid = pile(capi, kind, n, 3, 4.0, 3.0)
    plain = run(kind, bodies, sid, 8, 6)
    with world(kind, bodies, sid) as w:
        w.set_terrain(tm.bumpy_field(9, 7, 5), (-3.2, -1.3), (1.3, 1.1))
        w.set_terrain(None)
        with pytest.raises(capi.XpbdError):
            w.sample_terrain(np.zeros((1, 2)))
        advance(w, 8, 6)
        assert np.array_equal(w.download(), plain)
    assert not np.isnan(plain).any()


# ---- 3. GPU == model on a bumpy field that covers part of the scene ------------------------------------------------------
BUMPY_ORIGIN, BUMPY_CELL = (-8.0, -1.5), (1.3, 1.1)           # 9 x 7 samples: [-8, 2.4) x [-1.5, 5.1); the piles span [0, 5]^2


def bumpy_terrain(seed=11):
    return tm.bumpy_field(9, 7, seed), BUMPY_ORIGIN, BUMPY_CELL


@pytest.mark.parametrize("speed", [0.0, 3.0])
@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 96, 3), (capi.SCENE_MIXED_DROP, 120, 5)])
def test_gpu_equals_the_model_on_a_bumpy_field(kind, n, seed, speed):
    frames, substeps, ground_mu = 10, 6, 0.4
    rng = np.random.default_rng(seed)
    bodies, sid = pile(capi, kind, n, seed, 4.0, 3.0)
    bodies[:, 33] -= 0.4                                        # the lowest start in the ground
    mu = MUS[rng.integers(0, len(MUS), n)]
    terrain = bumpy_terrain()
    model = tm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[kind]), tm.Terrain(*terrain), mu=mu, ground_mu=ground_mu, pad=0.02,
                     max_depenetration_speed=speed)
    outside = contacts = 0
    for _ in range(frames):
        model.ground_trace = []
        want = model.step(DT, substeps).copy()
        contacts += len(model.ground_trace)
    for b in range(n):                                          # (a check of the scene) vertices beyond the edge, and bodies past it
        centre = want[b, 31:34] + want[b, 28:31]
        outside += tm.Terrain(*terrain).plane(tuple(centre)) is None
    print("%d ground constraints, %d of %d centres beyond the field" % (contacts, outside, n))
    assert contacts > 100 and 5 < outside < n - 5 and not np.isnan(want).any()
    got, masks, last = run(kind, bodies, sid, frames, substeps, terrain, mu, ground_mu, speed, masks=True)
    assert bits_equal(got, want)
    assert np.array_equal(masks[-1], np.array(model.masks, dtype=np.uint32))
    assert np.array_equal(last, ob.masks_to_contacts(np.array(model.masks, dtype=np.uint32)))
    assert not bits_equal(got, run(kind, bodies, sid, frames, substeps, PLANE, mu, ground_mu, speed))       # the terrain matters
    assert bits_equal(run(kind, bodies, sid, frames, substeps, terrain, mu, ground_mu, speed, split=True), want)


# ---- 4. restitution on terrain ------------------------------------------------------------------------------------------------
def test_box_dropped_on_a_tilted_field_bounces_as_the_model():
    kind, frames, substeps, e = capi.SCENE_BOXES, 30, 10, 0.5
    bodies, sid, _ = mm.resting_box(capi, 0.0, z=0.6)
    bodies[0, 31:33] = [0.3, 0.2]
    origin, cell = (-2.0, -2.0), (2.0, 2.0)
    terrain = tm.tilted_field(3, 3, origin, cell, 0.2, 0.05), origin, cell
    model = tm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[kind]), tm.Terrain(*terrain), e=[e], ground_e=e)
    vz = []
    for _ in range(frames):
        want = model.step(DT, substeps).copy()
        vz.append(want[0, 24])
    print("ground entries %d, vz min %.3f max %.3f" % (model.ground_entries, min(vz), max(vz)))
    assert model.ground_entries > 0 and min(vz) < -2.0 and max(vz) > 0.0 and not np.isnan(want).any()      # it fell, and it did bounce
    assert bits_equal(run(kind, bodies, sid, frames, substeps, terrain, e=[e], ground_e=e), want)
    flat = tm.flat_field(3, 3), origin, cell
    assert np.array_equal(run(kind, bodies, sid, frames, substeps, flat, e=[e], ground_e=e),
                          run(kind, bodies, sid, frames, substeps, PLANE, e=[e], ground_e=e))


# ---- 5. physics: a real slope under plain gravity ---------------------------------------------------------------------------
@pytest.mark.parametrize("tan_theta,sticks", [(0.25, True), (1.0, False)])
def test_box_on_a_tilted_field_sticks_below_and_slides_above_the_friction_angle(tan_theta, sticks):
    """material_model.STICKS / SLIDES, the thresholds of the same experiment with tilted gravity.  The model's creep on the real
    slope, measured: 3.75 mm of 1.190 m in 1 s (0.32 %) at tan(theta) = 0.25, mu = 0.5 -- below STICKS / 3 = 1.67 %, so the
    constant stands; at tan(theta) = 1.0 it slides 1.736 m of 3.468 m (Coulomb: half)."""
    bodies, sid, theta, downhill = tm.box_on_slope(capi, tan_theta)
    origin, cell = (-12.0, -3.0), (1.0, 1.0)
    terrain = tm.tilted_field(17, 8, origin, cell, tan_theta), origin, cell
    free = 0.5 * G * math.sin(theta)

    def verdict(d):
        return abs(d) < mm.STICKS * free if sticks else mm.SLIDES * free < d < (1.0 - mm.SLIDES) * free

    model = tm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES]), tm.Terrain(*terrain), mu=[0.5], ground_mu=INF)
    for _ in range(60):
        model.step(DT, 20)
    d_model = float(np.dot(model.bodies[0, 31:34] - bodies[0, 31:34], downhill))
    assert verdict(d_model)                                     # the model alone first
    got = run(capi.SCENE_BOXES, bodies, sid, 60, 20, terrain, [0.5], INF)
    d = float(np.dot(got[0, 31:34] - bodies[0, 31:34], downhill))
    print("tan(theta) %.2f: model %.4f m, device %.4f m of %.4f m" % (tan_theta, d_model, d, free))
    assert not np.isnan(got).any() and verdict(d)


# ---- 6. no tunnelling ---------------------------------------------------------------------------------------------------------
def test_nothing_tunnels_through_the_bumpy_field():
    """Every body whose centre is over the field stays above height(centre) - shape radius: a body all of whose vertices are on
    or above the surface has its centre (their mean, for these shapes) no lower than the lowest of them, and no vertex of it is
    further than the radius from the centre.  The field lies under the whole pile here, and the depenetration limit keeps the
    pile from bursting, so most bodies stay on it; a body that has once been past an edge is left out from then on (it falls,
    and drifting back below the surface would be no tunnelling)."""
    kind, n = capi.SCENE_BOXES_DROP, 96
    bodies, sid = pile(capi, kind, n, 3, 4.0, 3.0)
    heights, origin, cell = tm.bumpy_field(9, 7, 11), (-3.2, -0.8), (1.3, 1.1)            # [-3.2, 7.2) x [-0.8, 5.8) under [0, 5]^2
    polys = capi.scene_polytopes(kind)
    radius = np.array([np.linalg.norm(p["vertices"] - p["centroid"], axis=1).max() for p in polys])[sid]
    over = np.ones(n, dtype=bool)
    with world(kind, bodies, sid) as w:
        w.set_max_depenetration_speed(3.0)
        w.set_terrain(heights, origin, cell)
        for _ in range(60):
            w.step(DT, 6)
            got = w.download()
            centre = got[:, 31:34] + got[:, 28:31]
            ground = w.sample_terrain(centre[:, :2], normals=False)
            over &= ~np.isnan(ground)
    clearance = centre[over, 2] - ground[over] + radius[over]
    print("%d of %d centres always over the field, lowest clearance %.3f m" % (over.sum(), n, clearance.min()))
    assert not np.isnan(got).any() and over.sum() >= n // 3       # (a check of the scene: the field is 10.4 m x 6.6 m under a 5 m pile)
    assert (centre[over, 2] >= ground[over] - radius[over]).all()


# ---- 7. lifetime and errors -------------------------------------------------------------------------------------------------
def test_terrain_survives_upload_population_changes_and_history_restore():
    kind, n, substeps = capi.SCENE_BOXES_DROP, 96, 6
    bodies, sid = pile(capi, kind, n, 3, 4.0, 3.0)
    terrain = bumpy_terrain()
    want = run(kind, bodies, sid, 8, substeps, terrain)
    assert not bits_equal(want, run(kind, bodies, sid, 8, substeps))
    extra, extra_sid = pile(capi, kind, 8, 9, 4.0, 3.0)
    extra[:, 31] += 40.0                                        # beyond the field and everybody's reach: they fall freely
    with world(kind, extra, extra_sid) as w:
        w.set_terrain(*terrain)
        w.upload(bodies, sid)                                   # upload keeps the terrain
        advance(w, 4, substeps)
        first = w.add_bodies(extra, extra_sid)
        assert first == n
        w.remove_bodies(np.arange(n, n + 8))
        w.set_joints(np.zeros(0, dtype=capi.JOINT_DTYPE))
        w.set_materials(None, INF)
        w.set_mode(capi.MODE_FUSED)
        w.set_mode(capi.MODE_CONTACTS)
        w.history_push()
        advance(w, 4, substeps)
        assert bits_equal(w.download(), want)
        w.history_restore(0)
        advance(w, 4, substeps)                                 # stepping on from the restored state: the same run again
        assert bits_equal(w.download(), want)


def test_invalid_descriptors_are_rejected_and_the_previous_terrain_stays():
    kind, n, substeps = capi.SCENE_BOXES_DROP, 96, 6
    bodies, sid = pile(capi, kind, n, 3, 4.0, 3.0)
    heights, origin, cell = bumpy_terrain()
    want = run(kind, bodies, sid, 8, substeps, (heights, origin, cell))
    L = capi.hip_lib()
    nan, inf = heights.copy(), heights.copy()
    nan[3, 4], inf[0, 0] = np.nan, np.inf
    with world(kind, bodies, sid) as w:
        w.set_terrain(heights, origin, cell)
        advance(w, 4, substeps)
        for bad in ((heights[:1], origin, cell), (heights[:, :1], origin, cell), (np.zeros((2049, 2049)), origin, cell), (nan, origin, cell),
                    (inf, origin, cell), (heights, (np.nan, 0.0), cell), (heights, (0.0, np.inf), cell), (heights, origin, (0.0, 1.0)),
                    (heights, origin, (1.0, -1.0)), (heights, origin, (np.inf, 1.0)), (heights, origin, (1.0, np.nan))):
            with pytest.raises(capi.XpbdError) as e:
                w.set_terrain(*bad)
            assert e.value.code == capi.E_INVALID
        hf = capi.HEIGHTFIELD(9, 7, (C.c_double * 2)(*origin), (C.c_double * 2)(*cell), None)
        assert L.xpbd_world_set_terrain(w._h, C.byref(hf)) == capi.E_INVALID                  # NULL heights
        assert L.xpbd_world_sample_terrain(w._h, None, 1, None, None) == capi.E_INVALID
        advance(w, 4, substeps)
        assert bits_equal(w.download(), want)


def test_fused_mode_accepts_a_terrain_and_ignores_it():
    kind, n = capi.SCENE_BOXES_DROP, 300
    bodies, sid = pile(capi, kind, n, 4, 30.0, 2.0)
    plain = run(kind, bodies, sid, 10, 20, mode=capi.MODE_FUSED)
    assert bits_equal(run(kind, bodies, sid, 10, 20, (tm.bumpy_field(9, 7, 2), (-5.0, -5.0), (5.0, 7.0)), mode=capi.MODE_FUSED), plain)
    assert not np.isnan(plain).any()


# ---- 8. the headless driver ----------------------------------------------------------------------------------------------------
def test_headless_runs_on_rolling_terrain(tmp_path):
    dump = tmp_path / "poses.bin"
    p = subprocess.run([os.path.join(capi.LIB_DIR, "xpbd_headless"), "--mode", "contacts", "--bodies", "256", "--frames", "20", "--substeps", "10",
                        "--terrain", "waves:0.3:4", "--dump", str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    print(p.stdout)
    poses = np.fromfile(dump, dtype=np.float64).reshape(256, 38)
    assert np.isfinite(poses).all()
    assert poses[:, 33].min() > -1.0                            # nobody fell through: the field lies under the whole scene
