"""The jointed scenes of tests/xprec_joints_cases.py through the C ABI (World.set_joints, set_joint_limits; SAT): bit for bit
against the oracle where it can run the scene (no limits, no friction), and within K_JOINTS of the extended-precision model
on every scene, angular limits that bind in contact included -- on the eight-lanes-per-body path and, behind a far field, on
the one-lane-per-body path."""
import numpy as np
import pytest

import xprec_joints_cases as jc
import xprec_pairs_cases as pc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
SCENE_NAMES = list(jc.SCENES)
SCHEDULES = (capi.SAT_SCHEDULE_AUTO, capi.SAT_SCHEDULE_ONE_PASS, capi.SAT_SCHEDULE_TWO_PASS)


def run(name, schedule=capi.SAT_SCHEDULE_AUTO, far=0):
    """Every single-substep frame of the scene on the device, each from the trajectory's state at its start.  far: that many
    boxes on a 4 m grid 200 m away, behind the scene's bodies (test_gpu_xprec_pairs.run)."""
    t = jc.trajectory(name)
    n = len(t["sid"])
    extra, extra_sid = capi.scene_generate(capi.SCENE_BOXES, 9, far) if far else (np.zeros((0, 38)), np.zeros(0, dtype=np.uint32))
    if far:
        k = np.arange(far)
        extra[:, 31], extra[:, 32] = 200.0 + 4.0 * (k % 128), 4.0 * (k // 128)
        extra[:, 22:25] *= 0.3
    sid = np.concatenate([t["sid"], extra_sid]).astype(np.uint32)
    out = []
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.set_sat_schedule(schedule)
        for start, *_ in t["frames"]:
            w.upload(np.concatenate([start, extra]), sid)
            w.set_joints(t["joints"])
            if len(t["limits"]):
                w.set_joint_limits(t["limits"])
            if t["speed"]:
                w.set_max_depenetration_speed(t["speed"])
            if t["mu"] is not None:
                w.set_materials(np.concatenate([t["mu"], np.full(far, np.inf)]), t["ground_mu"])
            w.step(t["h"], 1)
            out.append(w.download()[:n])
    return t, out


def verdict(name, t, got):
    """The oracle's bits where it defines the scene; the model's bound and the exclusion caps on this run everywhere."""
    if name in jc.ORACLE_SCENES:
        for f, fr in enumerate(t["frames"]):
            assert bits_equal(got[f], fr[1]), "state differs from the oracle in substep %d" % f
    errs, excl, mixed = jc.check_states(name, got)
    jc.assert_caps(name, excl, mixed)
    print("%s: device against the model %.1f" % (name, np.where(excl, 0, errs).max()))
    return errs, excl


@pytest.mark.parametrize("schedule", SCHEDULES, ids=["auto", "one-pass", "two-pass"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_jointed_scenes(name, schedule):
    t, got = run(name, schedule=schedule)
    verdict(name, t, got)


@pytest.mark.parametrize("name", jc.LIMIT_SCENES + ["chain-h240-mu-limit3", "doors-h1200"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """The same verdicts with more than SMALL_WORLD bodies in the world, and the same bits as the small world's run: the
    one-lane path adds the same terms in the same order."""
    t, got = run(name, far=SMALL_WORLD + 16)
    verdict(name, t, got)
    _, small = run(name)
    for f in range(len(got)):
        assert bits_equal(got[f], small[f]), f


@pytest.mark.parametrize("name", jc.LIMIT_SCENES)
def test_limits_change_the_device_result(name):
    """Without set_joint_limits the device leaves the bound of the model with limits: the check sees the limits."""
    t = jc.trajectory(name)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        start, _, res, _ = t["frames"][0]
        w.upload(start, t["sid"])
        w.set_joints(t["joints"])
        w.step(t["h"], 1)
        got = w.download()
    e = np.where(jc.excluded(res), 0, jc.errors(name, got, res, start))
    assert e.max() > jc.K_JOINTS
