"""The scenes of tests/xprec_drives_cases.py through the C ABI (World.set_joints, set_joint_limits, set_joint_drives; SAT):
sliders, SLIDE limits and joint drives in contact within K_DRIVES of the extended-precision model on every scene and under
every SAT schedule, on the eight-lanes-per-body path and, behind a far field, on the one-lane-per-body path; the controls
without the drives and without the SLIDE limits; and the seam between a four-substep step and four single-substep steps."""
import numpy as np
import pytest

import xprec_check as xk
import xprec_device as xd
import xprec_drives_cases as dc
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(dc.SCENES)


def run(name, **kw):
    """Every single-substep frame of the scene on the device, each from the trajectory's state at its start."""
    t = dc.trajectory(name)
    return t, xd.run_frames([(fr[0], t) for fr in t["frames"]], **kw)


@pytest.mark.parametrize("schedule", xd.SAT_SCHEDULES, ids=xd.SCHEDULE_IDS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_driven_scenes(name, schedule):
    _, got = run(name, schedule=schedule)
    xd.verdict(dc, name, got)


@pytest.mark.parametrize("name", [n for n in SCENE_NAMES if n.startswith(("wheels", "mixed"))] + ["lifts-h1200"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """The same verdict with more than SMALL_WORLD bodies in the world, and the same bits as the small world's run: the pair
    solve changes its lane layout there, k_joint_extras does not."""
    _, got = run(name, far=xd.SMALL_WORLD + 16)
    xd.verdict(dc, name, got)
    _, small = run(name)
    for f in range(len(got)):
        assert bits_equal(got[f], small[f]), f


@pytest.mark.parametrize("without", ["drives", "slide limits"])
@pytest.mark.parametrize("name", ["lifts-h1200", "wheels-h1200"])
def test_the_extras_change_the_device_result(name, without):
    """Without set_joint_drives, and without the SLIDE limits, the device leaves the bound of the model that has them: the
    check sees the extras."""
    t, got = run(name, without=(without,), frames=1)
    start, _, res, _ = t["frames"][0]
    e = np.where(dc.excluded(res), 0, dc.errors(name, got[0], res, start))
    assert e.max() > dc.K_DRIVES


def test_four_substeps_in_one_step_equal_four_steps():
    """Scene (a) at h = 1/1200 from frame 0: step(4 h, 4) equals four step(h, 1) bit for bit, so the fused
    k_pair_solve_integrate_ground path hands the velocity drives the same `past` as the single-substep path that the model
    checks.  Printed beside it: the four-substep result against the model chained four times (a figure, no bound: the
    device's rounding of one substep is the next one's input)."""
    name = "lifts-h1200"
    t = dc.trajectory(name)
    start, h = t["frames"][0][0], t["h"]
    with xd.new_world() as w:
        fused, single, _ = xd.seam_runs(w, lambda: xd.prepare(w, t, start), h, split=False)
    state = start
    for _ in range(4):
        res = dc.model(name, state)
        state = res["state"]
    e = xk.scene_errors(t, fused, res, start)
    print("%s: four substeps against the model chained four times %.1f" % (name, e.max()))
    assert np.abs(fused - start)[:, 31:38].max() > 1e-4
    assert bits_equal(fused, single)
