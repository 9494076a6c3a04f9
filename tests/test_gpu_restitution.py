"""Restitution (xpbd_world_set_restitution) on the GPU: off, all zero or cleared it changes no bit (and equals the oracle); with
mixed coefficients the device equals the independent model (tests/restitution_model.py) bit for bit, alone and as an island of
a large world; xpbd_world_step equals the split API; the drop and head-on scenes keep the model's bounds; lifetime."""
import numpy as np
import pytest

import oracle_binding as ob
import restitution_model as rm
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, chain_joints, pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
ES = np.array([0.0, 0.3, 0.8, 1.0])
MUS = np.array([0.0, 0.2, 0.5, 1.0, np.inf])
NO_JOINTS = np.zeros(0, dtype=capi.JOINT_DTYPE)
PLAIN = "no set_restitution call"


def mixed_e(rng, n):
    return ES[rng.integers(0, len(ES), n)]


def world(kind, bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT):
    w = capi.World(mode=mode)
    w.set_polytopes(capi.scene_polytopes(kind))
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


def run(kind, bodies, sid, frames, substeps, e=PLAIN, ground_e=0.0, threshold=0.0, joints=None, narrowphase=capi.NARROWPHASE_SAT,
        mode=capi.MODE_CONTACTS, speed=0.0, mu=None, ground_mu=np.inf, split=False):
    with world(kind, bodies, sid, mode, narrowphase) as w:
        if joints is not None:
            w.set_joints(joints)
        if speed:
            w.set_max_depenetration_speed(speed)
        if mu is not None:
            w.set_materials(mu, ground_mu)
        if e is not PLAIN:
            w.set_restitution(e, ground_e, threshold)
        for _ in range(frames):
            if split:
                w.contacts_begin(DT)
                for _ in range(substeps):
                    w.contacts_substep(DT / substeps)
            else:
                w.step(DT, substeps)
        return w.download()


def with_far_field(bodies, sid, kind, count, seed):
    """test_gpu_materials.py's: the scene followed by `count` bodies 200 m away, so the scene keeps its indices."""
    far, far_sid = capi.scene_generate(kind, seed, count)
    k = np.arange(count)
    far[:, 31] = 200.0 + 4.0 * (k % 128)
    far[:, 32] = 4.0 * (k // 128)
    far[:, 22:25] *= 0.3
    return np.concatenate([bodies, far]), np.concatenate([sid, far_sid])


# ---- 3. off, zero and cleared change no bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
@pytest.mark.parametrize("big", [False, True])
def test_no_restitution_changes_no_bit(narrowphase, big):
    """The 160-box pile with chain joints of test_gpu_materials.py, alone or in front of 16 400 far-away bodies."""
    kind, n, frames, substeps = capi.SCENE_BOXES_DROP, 160, 12, 10
    bodies, sid = pile(capi, kind, n, 6, 4.0, 6.0)
    joints = chain_joints(capi, n)
    scene, scene_sid = with_far_field(bodies, sid, kind, SMALL_WORLD + 16, 9) if big else (bodies, sid)
    plain = run(kind, scene, scene_sid, frames, substeps, joints=joints, narrowphase=narrowphase)
    zeros = run(kind, scene, scene_sid, frames, substeps, np.zeros(len(scene)), 0.0, 0.0, joints=joints, narrowphase=narrowphase)
    cleared = run(kind, scene, scene_sid, frames, substeps, None, 0.0, 0.0, joints=joints, narrowphase=narrowphase)
    threshold_only = run(kind, scene, scene_sid, frames, substeps, None, 0.0, 0.5, joints=joints, narrowphase=narrowphase)
    assert not np.isnan(plain).any()
    assert bits_equal(zeros, plain) and bits_equal(cleared, plain) and bits_equal(threshold_only, plain)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    want, stats = bodies, ob.ContactStats()
    for _ in range(frames):
        want = ob.contacts_step_joints(want, sid, polys, joints, DT, substeps, 0.02, narrowphase=int(narrowphase), stats=stats)
    assert stats.n_points > 1000
    assert bits_equal(plain[:n], want)


# ---- 4. GPU == model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materials", [False, True])
@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 96, 3), (capi.SCENE_MIXED_DROP, 120, 5)])
def test_gpu_equals_the_model_with_mixed_coefficients(kind, n, seed, materials):
    """Coefficients from {0, 0.3, 0.8, 1}, ground 0.5; with and without friction materials and the depenetration limit."""
    frames, substeps, ground_e = 8, 6, 0.5
    rng = np.random.default_rng(seed)
    bodies, sid = pile(capi, kind, n, seed, 4.0, 3.0)
    e = mixed_e(rng, n)
    mu, ground_mu, speed = (MUS[rng.integers(0, len(MUS), n)], 0.4, 3.0) if materials else (None, np.inf, 0.0)
    model = rm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[kind]), e, ground_e, 0.0, mu=mu, ground_mu=ground_mu, pad=0.02,
                     max_depenetration_speed=speed)
    for _ in range(frames):
        want = model.step(DT, substeps)
    print("model: %d pair entries, %d ground entries" % (model.pair_entries, model.ground_entries))
    assert model.pair_entries >= 1 and model.ground_entries >= 1      # otherwise the comparison proves nothing
    got = run(kind, bodies, sid, frames, substeps, e, ground_e, speed=speed, mu=mu, ground_mu=ground_mu)
    assert not np.isnan(want).any()
    assert bits_equal(got, want)
    assert not bits_equal(got, run(kind, bodies, sid, frames, substeps, speed=speed, mu=mu, ground_mu=ground_mu))   # it matters
    # the same bodies as an island in a world beyond the eight-lanes-per-body size
    scene, scene_sid = with_far_field(bodies, sid, kind, SMALL_WORLD + 16, 11)
    far = len(scene) - n
    island = run(kind, scene, scene_sid, frames, substeps, np.concatenate([e, mixed_e(rng, far)]), ground_e, speed=speed,
                 mu=None if mu is None else np.concatenate([mu, MUS[rng.integers(0, len(MUS), far)]]), ground_mu=ground_mu)
    assert bits_equal(island[:n], got)


# ---- 5. step == begin + n x substep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
def test_step_equals_the_split_api_with_restitution(narrowphase):
    kind, n = capi.SCENE_MIXED_DROP, 300
    bodies, sid = pile(capi, kind, n, 8, 5.0, 4.0)
    e = mixed_e(np.random.default_rng(8), n)
    joints = chain_joints(capi, n)
    whole = run(kind, bodies, sid, 10, 6, e, 0.5, 0.05, joints=joints, narrowphase=narrowphase)
    split = run(kind, bodies, sid, 10, 6, e, 0.5, 0.05, joints=joints, narrowphase=narrowphase, split=True)
    assert not np.isnan(whole).any() and bits_equal(whole, split)
    assert not bits_equal(whole, run(kind, bodies, sid, 10, 6, joints=joints, narrowphase=narrowphase))


# ---- 6. physics through the ABI, the model's scenes and bounds -----------------------------------------------------------------
def drop(e, ground_e=0.0, frames=110):
    bodies, sid = rm.dropped_box(capi, rm.DROP_HEIGHT)
    z, vz = [], []
    with world(capi.SCENE_BOXES, bodies, sid) as w:
        w.set_restitution([e], ground_e, 0.0)
        for _ in range(frames):
            w.step(DT, 20)
            got = w.download()
            z.append(float(got[0, 33]))
            vz.append(float(got[0, 24]))
    return z, vz, got


@pytest.mark.parametrize("e", [0.5, 0.8])
def test_dropped_box_bounces_by_its_coefficient(e):
    z, vz, _ = drop(e)
    k = rm.bounce_frame(vz)
    ratio, apex = -vz[k] / vz[k - 1], rm.apex_after(z, k)
    print("drop e %.1f: frame %d, %.4f -> %.4f m/s, ratio %.4f; apex %.4f m of %.4f m" % (e, k, vz[k - 1], vz[k], ratio, apex,
                                                                                          e * e * rm.DROP_HEIGHT))
    assert abs(ratio - e) < rm.DROP_RATIO_BOUND
    assert abs(apex / (e * e * rm.DROP_HEIGHT) - 1.0) < rm.DROP_APEX_BOUND


def test_contact_takes_the_larger_coefficient():
    want = drop(0.9, 0.9, 60)[2]
    assert bits_equal(drop(0.2, 0.9, 60)[2], want) and bits_equal(drop(0.9, 0.0, 60)[2], want)
    z, vz, got = drop(0.2, 0.0, 60)
    assert not bits_equal(got, want)
    k = rm.bounce_frame(vz)
    assert abs(-vz[k] / vz[k - 1] - 0.2) < rm.DROP_RATIO_BOUND


def test_box_at_rest_under_a_bounce_threshold_stays_at_rest_to_the_bit():
    bodies, sid = rm.dropped_box(capi, 0.0)
    still = run(capi.SCENE_BOXES, bodies, sid, 30, 20)
    assert bits_equal(run(capi.SCENE_BOXES, bodies, sid, 30, 20, [0.8], 0.8, 1.0), still)
    assert not bits_equal(run(capi.SCENE_BOXES, bodies, sid, 30, 20, [0.8], 0.8, 0.0), still)


@pytest.mark.parametrize("e", [1.0, 0.5])
def test_boxes_head_on_leave_at_e_times_the_closing_speed_and_keep_their_momentum(e):
    bodies, sid = rm.head_on_boxes(capi, 1.0)
    got = run(capi.SCENE_BOXES, bodies, sid, 40, 20, [e, e])
    ratio = (got[1, 22] - got[0, 22]) / 2.0
    print("head-on e %.1f: velocities %.6f, %.6f m/s; relative speed after / before %.4f; momentum %.3e" % (e, got[0, 22], got[1, 22], ratio,
                                                                                                          got[0, 22] + got[1, 22]))
    assert got[0, 22] < 0.0 < got[1, 22]
    assert abs(got[0, 22] + got[1, 22]) < rm.HEAD_ON_MOMENTUM_BOUND
    assert np.abs(got[:, 23:28]).max() < rm.HEAD_ON_SPIN_BOUND
    assert abs(ratio - e) < rm.HEAD_ON_BOUND[e]                                          # e = 1: velocities exchanged; 0.5: halved


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------------
def test_upload_resets_restitution_and_joints_materials_and_history_leave_it_alone():
    kind, n, substeps = capi.SCENE_BOXES_DROP, 200, 6
    bodies, sid = pile(capi, kind, n, 7, 4.0, 3.0)
    e = mixed_e(np.random.default_rng(1), n)
    want = run(kind, bodies, sid, 12, substeps, e, 0.5, 0.02)
    plain = run(kind, bodies, sid, 12, substeps)
    assert not np.isnan(want).any() and not bits_equal(want, plain)
    with world(kind, bodies, sid) as w:
        w.set_restitution(e, 0.5, 0.02)
        for _ in range(4):
            w.step(DT, substeps)
        w.set_joints(NO_JOINTS)
        w.set_materials(None, np.inf)
        for _ in range(4):
            w.step(DT, substeps)
        # history restore + re-step reproduces a bouncing run bit for bit
        w.history_push()
        for _ in range(4):
            w.step(DT, substeps)
        assert bits_equal(w.download(), want)
        w.history_restore(0)
        for _ in range(4):
            w.step(DT, substeps)
        assert bits_equal(w.download(), want)
        w.upload(bodies, sid)                                          # resets
        for _ in range(12):
            w.step(DT, substeps)
        assert bits_equal(w.download(), plain)


@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
def test_pinned_modes_accept_restitution_and_ignore_it(mode):
    kind, n = capi.SCENE_BOXES_DROP, 300
    bodies, sid = pile(capi, kind, n, 4, 30.0, 2.0)
    plain = run(kind, bodies, sid, 10, 20, mode=mode)
    assert bits_equal(run(kind, bodies, sid, 10, 20, mixed_e(np.random.default_rng(3), n), 1.0, 0.0, mode=mode), plain)
    assert not np.isnan(plain).any()


def test_contact_reports_are_the_same_bytes_with_zero_restitution():
    kind, n = capi.SCENE_BOXES_DROP, 300
    bodies, sid = pile(capi, kind, n, 5, 4.0, 4.0)
    out = []
    for e in (PLAIN, np.zeros(n)):
        with world(kind, bodies, sid) as w:
            w.set_contact_report(True)
            if e is not PLAIN:
                w.set_restitution(e, 0.0, 0.0)
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
