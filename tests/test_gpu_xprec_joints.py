"""The jointed scenes of tests/xprec_joints_cases.py through the C ABI (World.set_joints, set_joint_limits; SAT): bit for bit
against the oracle where it can run the scene (no limits, no friction), and within K_JOINTS of the extended-precision model
on every scene, angular limits that bind in contact included -- on the eight-lanes-per-body path and, behind a far field, on
the one-lane-per-body path."""
import numpy as np
import pytest

import xprec_device as xd
import xprec_joints_cases as jc
import xprec_pairs_cases as pc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(jc.SCENES)


def run(name, **kw):
    """Every single-substep frame of the scene on the device, each from the trajectory's state at its start."""
    t = jc.trajectory(name)
    return t, xd.run_frames([(fr[0], t) for fr in t["frames"]], **kw)


def verdict(name, t, got):
    """The oracle's bits where it defines the scene; the model's bound and the exclusion caps on this run everywhere."""
    if name in jc.ORACLE_SCENES:
        for f, fr in enumerate(t["frames"]):
            assert bits_equal(got[f], fr[1]), "state differs from the oracle in substep %d" % f
    xd.verdict(jc, name, got)


@pytest.mark.parametrize("schedule", xd.SAT_SCHEDULES, ids=xd.SCHEDULE_IDS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_jointed_scenes(name, schedule):
    t, got = run(name, schedule=schedule)
    verdict(name, t, got)


@pytest.mark.parametrize("name", jc.LIMIT_SCENES + ["chain-h240-mu-limit3", "doors-h1200"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """The same verdicts with more than SMALL_WORLD bodies in the world, and the same bits as the small world's run: the
    one-lane path adds the same terms in the same order."""
    t, got = run(name, far=xd.SMALL_WORLD + 16)
    verdict(name, t, got)
    _, small = run(name)
    for f in range(len(got)):
        assert bits_equal(got[f], small[f]), f


@pytest.mark.parametrize("name", jc.LIMIT_SCENES)
def test_limits_change_the_device_result(name):
    """Without set_joint_limits the device leaves the bound of the model with limits: the check sees the limits."""
    t = jc.trajectory(name)
    start, _, res, _ = t["frames"][0]
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        w.upload(start, t["sid"])
        w.set_joints(t["joints"])
        w.step(t["h"], 1)
        got = w.download()
    e = np.where(jc.excluded(res), 0, jc.errors(name, got, res, start))
    assert e.max() > jc.K_JOINTS
