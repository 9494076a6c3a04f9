"""The scenes of tests/xprec_drives_cases.py through the C ABI (World.set_joints, set_joint_limits, set_joint_drives; SAT):
sliders, SLIDE limits and joint drives in contact within K_DRIVES of the extended-precision model on every scene and under
every SAT schedule, on the eight-lanes-per-body path and, behind a far field, on the one-lane-per-body path; the controls
without the drives and without the SLIDE limits; and the seam between a four-substep step and four single-substep steps."""
import numpy as np
import pytest

import xprec_drives_cases as dc
import xprec_pairs_cases as pc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
SCENE_NAMES = list(dc.SCENES)
SCHEDULES = (capi.SAT_SCHEDULE_AUTO, capi.SAT_SCHEDULE_ONE_PASS, capi.SAT_SCHEDULE_TWO_PASS)


def far_field(far):
    """That many boxes on a 4 m grid 200 m away (test_gpu_xprec_joints.run)."""
    if not far:
        return np.zeros((0, 38)), np.zeros(0, dtype=np.uint32)
    extra, extra_sid = capi.scene_generate(capi.SCENE_BOXES, 9, far)
    k = np.arange(far)
    extra[:, 31], extra[:, 32] = 200.0 + 4.0 * (k % 128), 4.0 * (k // 128)
    extra[:, 22:25] *= 0.3
    return extra, extra_sid


def prepare(w, t, start, extra, sid, without=()):
    w.upload(np.concatenate([start, extra]), sid)
    w.set_joints(t["joints"])
    limits = t["limits"][t["limits"]["kind"] != capi.LIMIT_SLIDE] if "slide limits" in without else t["limits"]
    if len(limits):
        w.set_joint_limits(limits)
    if len(t["drives"]) and "drives" not in without:
        w.set_joint_drives(t["drives"])
    if t["speed"]:
        w.set_max_depenetration_speed(t["speed"])
    if t["mu"] is not None:
        w.set_materials(np.concatenate([t["mu"], np.full(len(extra), np.inf)]), t["ground_mu"])


def run(name, schedule=capi.SAT_SCHEDULE_AUTO, far=0, without=(), frames=None):
    """Every single-substep frame of the scene on the device, each from the trajectory's state at its start."""
    t = dc.trajectory(name)
    n = len(t["sid"])
    extra, extra_sid = far_field(far)
    sid = np.concatenate([t["sid"], extra_sid]).astype(np.uint32)
    out = []
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.set_sat_schedule(schedule)
        for start, *_ in t["frames"][:frames]:
            prepare(w, t, start, extra, sid, without)
            w.step(t["h"], 1)
            out.append(w.download()[:n])
    return t, out


def verdict(name, got):
    """The model's bound and the exclusion caps on this run."""
    errs, excl, mixed = dc.check_states(name, got)
    dc.assert_caps(name, excl, mixed)
    print("%s: device against the model %.1f" % (name, np.where(excl, 0, errs).max()))


@pytest.mark.parametrize("schedule", SCHEDULES, ids=["auto", "one-pass", "two-pass"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_driven_scenes(name, schedule):
    _, got = run(name, schedule=schedule)
    verdict(name, got)


@pytest.mark.parametrize("name", [n for n in SCENE_NAMES if n.startswith(("wheels", "mixed"))] + ["lifts-h1200"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """The same verdict with more than SMALL_WORLD bodies in the world, and the same bits as the small world's run: the pair
    solve changes its lane layout there, k_joint_extras does not."""
    _, got = run(name, far=SMALL_WORLD + 16)
    verdict(name, got)
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
    none = far_field(0)[0]
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        prepare(w, t, start, none, t["sid"])
        w.step(4 * h, 4)
        fused = w.download()
        prepare(w, t, start, none, t["sid"])
        for _ in range(4):
            w.step(h, 1)
        single = w.download()
    state = start
    for _ in range(4):
        res = dc.model(name, state)
        state = res["state"]
    e = pc.normalized_errors(fused, state, start, t["ext"], h, dc.links(name, res))
    print("%s: four substeps against the model chained four times %.1f" % (name, e.max()))
    assert np.abs(fused - start)[:, 31:38].max() > 1e-4
    assert bits_equal(fused, single)
