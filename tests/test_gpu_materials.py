"""Contact materials (xpbd_world_set_materials, xpbd_multi_world_set_materials) on the GPU: materials that are off or all +inf
change no bit (and equal the oracle); with finite, mixed coefficients the device equals the independent model
(tests/material_model.py) bit for bit, on both pair-solve paths; a box sticks or slides on a slope, on the ground and on a
static slab body, by the smaller coefficient of the two sides; a frictionless floor keeps the horizontal speed; a sharded
world equals the single one through re-plans that move bodies between owners; lifetime and errors."""
import math

import numpy as np
import pytest

import material_model as mm
import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, chain_joints, line_scene, pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
G = 9.81
INF = np.inf
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
MUS = np.array([0.0, 0.2, 0.5, 1.0, INF])
NO_JOINTS = np.zeros(0, dtype=capi.JOINT_DTYPE)


def mixed_mu(rng, n):
    return MUS[rng.integers(0, len(MUS), n)]


def world(kind, bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT, polys=None):
    w = capi.World(mode=mode)
    w.set_polytopes(capi.scene_polytopes(kind) if polys is None else polys)
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


PLAIN = "no set_materials call"


def run(kind, bodies, sid, frames, substeps, mu=PLAIN, ground_mu=INF, joints=None, narrowphase=capi.NARROWPHASE_SAT, mode=capi.MODE_CONTACTS,
        speed=0.0, polys=None):
    with world(kind, bodies, sid, mode, narrowphase, polys) as w:
        if joints is not None:
            w.set_joints(joints)
        if speed:
            w.set_max_depenetration_speed(speed)
        if mu is not PLAIN:
            w.set_materials(mu, ground_mu)
        for _ in range(frames):
            w.step(DT, substeps)
        return w.download()


def with_far_field(bodies, sid, kind, count, seed):
    """The scene followed by `count` bodies of the same kind on a 4 m grid 200 m away: nothing of it can reach the scene, and
    the scene keeps its indices, so its Jacobi sums keep their order."""
    far, far_sid = capi.scene_generate(kind, seed, count)
    k = np.arange(count)
    far[:, 31] = 200.0 + 4.0 * (k % 128)
    far[:, 32] = 4.0 * (k // 128)
    far[:, 22:25] *= 0.3
    return np.concatenate([bodies, far]), np.concatenate([sid, far_sid])


# ---- 1. off and +inf change no bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
@pytest.mark.parametrize("big,per_body_mass", [(False, True), (True, False)])
def test_materials_off_or_infinite_change_no_bit(narrowphase, big, per_body_mass):
    """A pile of 160 boxes with ground and pair contacts and chain joints, alone (eight lanes per body) or in front of 16 400
    far-away bodies (one lane per body); mass properties shared per shape, or per body (one body is heavier)."""
    kind, n, frames, substeps = capi.SCENE_BOXES_DROP, 160, 12, 10
    bodies, sid = pile(capi, kind, n, 6, 4.0, 6.0)
    if per_body_mass:
        bodies[7, 0] *= 0.5
    joints = chain_joints(capi, n)
    scene, scene_sid = with_far_field(bodies, sid, kind, SMALL_WORLD + 16, 9) if big else (bodies, sid)
    total = len(scene)
    plain = run(kind, scene, scene_sid, frames, substeps, joints=joints, narrowphase=narrowphase)
    infinite = run(kind, scene, scene_sid, frames, substeps, np.full(total, INF), INF, joints=joints, narrowphase=narrowphase)
    cleared = run(kind, scene, scene_sid, frames, substeps, None, INF, joints=joints, narrowphase=narrowphase)
    ground_only = run(kind, scene, scene_sid, frames, substeps, None, 1e300, joints=joints, narrowphase=narrowphase)
    assert not np.isnan(plain).any()
    assert bits_equal(infinite, plain) and bits_equal(cleared, plain)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    want, stats = bodies, ob.ContactStats()
    for _ in range(frames):
        want = ob.contacts_step_joints(want, sid, polys, joints, DT, substeps, 0.02, narrowphase=int(narrowphase), stats=stats)
    assert stats.n_points > 1000
    assert bits_equal(plain[:n], want)
    # (a ground coefficient no contact can reach runs the kernels' material forms on every body as well)
    assert bits_equal(ground_only, plain)


# ---- 2. GPU == model, 3. the same bits on both pair-solve paths ----------------------------------------------------------------
@pytest.mark.parametrize("speed", [0.0, 3.0])
@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 96, 3), (capi.SCENE_MIXED_DROP, 120, 5)])
def test_gpu_equals_the_model_with_mixed_coefficients_on_both_pair_solve_paths(kind, n, seed, speed):
    frames, substeps, ground_mu = 10, 6, 0.4
    rng = np.random.default_rng(seed)
    bodies, sid = pile(capi, kind, n, seed, 4.0, 3.0)
    mu = mixed_mu(rng, n)
    model = mm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[kind]), mu, ground_mu, pad=0.02, max_depenetration_speed=speed)
    for _ in range(frames):
        want = model.step(DT, substeps)
    got = run(kind, bodies, sid, frames, substeps, mu, ground_mu, speed=speed)
    assert not np.isnan(want).any()
    assert bits_equal(got, want)
    assert not bits_equal(got, run(kind, bodies, sid, frames, substeps, speed=speed))     # the coefficients matter
    # the same bodies as an island in a world beyond the eight-lanes-per-body size
    scene, scene_sid = with_far_field(bodies, sid, kind, SMALL_WORLD + 16, 11)
    far_mu = np.concatenate([mu, mixed_mu(rng, len(scene) - n)])
    island = run(kind, scene, scene_sid, frames, substeps, far_mu, ground_mu, speed=speed)
    assert bits_equal(island[:n], got)


# ---- 4. physics through the ABI ---------------------------------------------------------------------------------------------
def moved(bodies, sid, mu, ground_mu, frames, polys=None):
    got = run(capi.SCENE_BOXES, bodies, sid, frames, 20, mu, ground_mu, polys=polys)
    assert not np.isnan(got).any()
    return got[0, 31] - bodies[0, 31], got


@pytest.mark.parametrize("mu,ground_mu", [(0.5, INF), (INF, 0.5)])
def test_box_on_a_slope_sticks_below_and_slides_above_the_friction_angle(mu, ground_mu):
    for tan_theta, sticks in ((0.25, True), (1.0, False)):
        bodies, sid, theta = mm.resting_box(capi, tan_theta)
        d, _ = moved(bodies, sid, [mu], ground_mu, 60)
        free = 0.5 * G * math.sin(theta)
        print("ground: tan(theta) %.2f moved %.4f m of %.4f m" % (tan_theta, d, free))
        if sticks:
            assert abs(d) < mm.STICKS * free
        else:
            assert mm.SLIDES * free < d < (1.0 - mm.SLIDES) * free


@pytest.mark.parametrize("tan_theta,mus,verdict", [(0.25, [0.5, 0.5], "sticks"), (1.0, [0.5, 0.5], "slides"), (0.5, [0.0, 1.0], "free"),
                                                   (0.5, [1.0, 0.0], "free"), (0.5, [1.0, 1.0], "sticks")])
def test_box_on_a_static_slab_body_takes_the_smaller_coefficient(tan_theta, mus, verdict):
    """The pair path carries the friction: the box rests on a static body (inverse mass 0), not on the ground."""
    bodies, sid, theta, polys = mm.box_on_slab(capi, tan_theta)
    d, got = moved(bodies, sid, mus, 0.0, 30, polys)             # (an icy ground: nothing touches it)
    free = 0.5 * G * math.sin(theta) * 0.25
    print("slab: tan(theta) %.2f mu %s moved %.4f m of %.4f m" % (tan_theta, mus, d, free))
    assert bits_equal(got[1], bodies[1])
    if verdict == "sticks":
        assert abs(d) < mm.STICKS * free
    elif verdict == "slides":
        assert mm.SLIDES * free < d < (1.0 - mm.SLIDES) * free
    else:
        assert d > (1.0 - mm.STICKS) * free


@pytest.mark.parametrize("mu,ground_mu", [(0.0, 1.0), (1.0, 0.0)])
def test_box_launched_along_a_frictionless_floor_keeps_its_speed(mu, ground_mu):
    """The ground's impulses have no horizontal part, so the only error of the horizontal velocity is the rounding of
    (pos - past) / h: about 1e-12 relative per substep at these magnitudes, over 1 200 substeps -- within 1e-6."""
    bodies, sid, _ = mm.resting_box(capi, 0.0)
    bodies[0, 22:25] = [2.0, 0.5, 0.0]
    got = run(capi.SCENE_BOXES, bodies, sid, 60, 20, [mu], ground_mu)
    start, end = math.hypot(2.0, 0.5), math.hypot(got[0, 22], got[0, 23])
    print("launched: speed %.15g -> %.15g (relative %.3e), z %.3e" % (start, end, abs(end - start) / start, got[0, 33]))
    assert abs(end - start) / start < 1e-6
    assert abs(got[0, 33]) < 1e-3 and abs(got[0, 31] - 2.0) < 1e-5      # still on the floor, one second further
    sticky = run(capi.SCENE_BOXES, bodies, sid, 60, 20)                # the reference's contact stops it dead
    assert math.hypot(sticky[0, 22], sticky[0, 23]) < 0.05 * start


# ---- 5. sharded == single -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_sharded_world_with_materials_equals_single(n_ranks):
    """test_gpu_collision_filter.py's migrating scene: a long line of spinning bodies that drifts across the cuts."""
    kind, n, substeps, frames, ground_mu = capi.SCENE_BOXES_DROP, 96, 6, 30, 0.3
    rng = np.random.default_rng(n_ranks)
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 25:28] = rng.normal(scale=6.0, size=(n, 3))
    bodies[:, 22] += 1.5
    joints = chain_joints(capi, n, every=1, distance=0.0, limit=n // 2)
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    mu = mixed_mu(rng, n)
    one = run(kind, bodies, sid, frames, substeps, mu, ground_mu, joints=joints)
    assert not bits_equal(one, run(kind, bodies, sid, frames, substeps, joints=joints))
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        mw.set_materials(mu, ground_mu)
        migrated = 0
        for f in range(frames):
            mw.step(DT, substeps)
            if f % 6 == 5:
                mw.replan()
                migrated += mw.plan_stats()["migrated"]
        got = mw.download()
        stats = mw.plan_stats()
    assert stats["plans"] > 1 and migrated > 0
    assert not np.isnan(one).any() and bits_equal(got, one)


def test_multi_world_takes_materials_before_the_plan_rejects_bad_ones_and_upload_resets_them():
    kind, n = capi.SCENE_BOXES_DROP, 64
    bodies, sid = line_scene(capi, kind, n, 4, 1.05)
    mu = mixed_mu(np.random.default_rng(2), n)
    with_mu = run(kind, bodies, sid, 8, 6, mu, 0.3)
    plain = run(kind, bodies, sid, 8, 6)
    assert not bits_equal(with_mu, plain)
    L = capi.hip_lib()
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=2.0, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n)
        mw.set_materials(mu, 0.3)
        bad = mu.copy()
        bad[5] = -0.1
        for materials, ground in ((mu[:-1], 0.3), (bad, 0.3), (mu, -1.0), (mu, np.nan)):
            with pytest.raises(capi.XpbdError) as e:
                mw.set_materials(materials, ground)
            assert e.value.code == capi.E_INVALID
        assert L.xpbd_multi_world_set_materials(mw._h, None, n, 0.3) == capi.E_INVALID
        for _ in range(8):
            mw.step(DT, 6)
        assert bits_equal(mw.download(), with_mu)
        mw.upload(bodies, sid, 0, n)                                   # resets the materials
        for _ in range(8):
            mw.step(DT, 6)
        assert bits_equal(mw.download(), plain)


# ---- 6. lifecycle and errors ------------------------------------------------------------------------------------------------
def test_bad_materials_are_rejected_and_the_previous_ones_stay():
    kind, n, substeps = capi.SCENE_BOXES_DROP, 200, 6
    rng = np.random.default_rng(1)
    bodies, sid = pile(capi, kind, n, 7, 4.0, 3.0)
    mu, ground_mu = mixed_mu(rng, n), 0.4
    want = run(kind, bodies, sid, 12, substeps, mu, ground_mu)
    plain = run(kind, bodies, sid, 12, substeps)
    assert not bits_equal(want, plain)
    L = capi.hip_lib()
    records = capi._materials(mu)
    with world(kind, bodies, sid) as w:
        w.set_materials(mu, ground_mu)
        for _ in range(4):
            w.step(DT, substeps)
        negative, nan, reserved = records.copy(), records.copy(), records.copy()
        negative["friction"][3], nan["friction"][n - 1], reserved["reserved"][0] = -1e-300, np.nan, 1.0
        for materials, ground in ((records[:-1], ground_mu), (np.concatenate([records, records[:1]]), ground_mu), (negative, ground_mu),
                                  (nan, ground_mu), (reserved, ground_mu), (records, -0.5), (records, np.nan), (None, -1.0)):
            with pytest.raises(capi.XpbdError) as e:
                w.set_materials(materials, ground)
            assert e.value.code == capi.E_INVALID
        assert L.xpbd_world_set_materials(w._h, None, n, ground_mu) == capi.E_INVALID
        for _ in range(4):
            w.step(DT, substeps)
        # set_joints and history push / restore leave the materials alone
        w.set_joints(NO_JOINTS)
        w.history_push()
        w.step(DT, substeps)
        w.history_restore(0)
        for _ in range(4):
            w.step(DT, substeps)
        assert bits_equal(w.download(), want)
        # upload resets them
        w.upload(bodies, sid)
        for _ in range(12):
            w.step(DT, substeps)
        assert bits_equal(w.download(), plain)


@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
def test_pinned_modes_accept_materials_and_ignore_them(mode):
    kind, n = capi.SCENE_BOXES_DROP, 300
    bodies, sid = pile(capi, kind, n, 4, 30.0, 2.0)
    mu = mixed_mu(np.random.default_rng(3), n)
    plain = run(kind, bodies, sid, 10, 20, mode=mode)
    assert bits_equal(run(kind, bodies, sid, 10, 20, mu, 0.0, mode=mode), plain)
    assert not np.isnan(plain).any()


def test_contact_reports_are_the_same_with_infinite_materials():
    kind, n = capi.SCENE_BOXES_DROP, 300
    bodies, sid = pile(capi, kind, n, 5, 4.0, 4.0)
    out = []
    for materials in (PLAIN, np.full(n, INF)):
        with world(kind, bodies, sid) as w:
            w.set_contact_report(True)
            if materials is not PLAIN:
                w.set_materials(materials, INF)
            events = []
            for _ in range(6):
                w.step(DT, 6)
                events.append(w.contact_events())
            pairs, points = w.pair_contacts()
            out.append((w.contact_report_counts(), pairs, points, events, w.download()))
    (counts_a, pairs_a, points_a, events_a, state_a), (counts_b, pairs_b, points_b, events_b, state_b) = out
    assert counts_a[0] > 50 and list(counts_a) == list(counts_b)
    assert pairs_a.tobytes() == pairs_b.tobytes() and points_a.tobytes() == points_b.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(events_a, events_b))
    assert bits_equal(state_a, state_b)
