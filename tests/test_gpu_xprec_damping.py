"""The scenes of tests/xprec_damping_cases.py through the C ABI (World.set_damping, set_joint_damping, set_kinematics with
set_restitution, set_materials, set_joints, set_joint_limits, set_joint_drives; SAT): stage 7 and the kinematic overwrite within
the bound of the extended-precision model on every scene and under every SAT schedule, on the eight-lanes-per-body path and,
behind a far field, on the one-lane-per-body path; the controls without each setter; the seams between a four-substep step,
four single-substep steps and the split API; the lone POSE entries over S substeps within the model's own bound; and scene (f)
in a world whose mass rows were edited in place."""
import numpy as np
import pytest

import xprec_check as xk
import xprec_damping_cases as dcs
import xprec_device as xd
import xprec_model as xm
import xprec_pairs_cases as pc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(dcs.SCENES)


def run(name, **kw):
    """Every single-substep frame of the scene on the device, each from the scene's state at its start."""
    t = dcs.trajectory(name)
    return t, xd.run_frames([(fr[0], fr[3]) for fr in t["frames"]], **kw)


@pytest.mark.parametrize("schedule", xd.SAT_SCHEDULES, ids=xd.SCHEDULE_IDS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_damped_and_kinematic_scenes(name, schedule):
    _, got = run(name, schedule=schedule)
    xd.verdict(dcs, name, got)


@pytest.mark.parametrize("name", ["drag-h1200", "jointed-h240", "chain-h1200", "platforms-h240"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """Scenes (a), (c) and (e) with more than SMALL_WORLD bodies in the world: the same verdict, and the small world's bits."""
    _, got = run(name, far=xd.SMALL_WORLD + 16)
    xd.verdict(dcs, name, got)
    _, small = run(name)
    for f in range(len(got)):
        assert bits_equal(got[f], small[f]), f


@pytest.mark.parametrize("name,without", [("drag-h1200", "damping"), ("caps-h1200", "damping"), ("jointed-h1200", "joint_damping"),
                                          ("chain-h1200", "joint_damping"), ("platforms-h1200", "kinematics")])
def test_without_the_setter_the_device_leaves_the_bound(name, without):
    """Without set_damping on (a) and (b), without set_joint_damping on (c), without set_kinematics on (e); two frames each."""
    t, got = run(name, without=(without,), frames=2)
    worst = 0.0
    for f in range(2):
        _, _, res, s = t["frames"][f]
        worst = max(worst, np.where(dcs.excluded(res, s), 0, dcs.errors(name, f, got[f], res) / dcs.bounds(res)).max())
    print("%s without %s: %.3g x the bound" % (name, without, worst))
    assert worst > 1.0


@pytest.mark.parametrize("name", ["drag-h1200", "caps-h1200", "jointed-h1200", "chain-h1200"])
def test_four_substeps_in_one_step_equal_four_steps_and_the_split_api(name):
    """From frame 0: step(4 h, 4) equals four step(h, 1) and contacts_begin + 4 x contacts_substep bit for bit, so every schedule
    runs stage 7 where the single-substep path that the model checks runs it.  Printed beside it: the four-substep result against
    the model chained four times (a figure, no bound).
    `chain` is held to the split API alone.  Its rods start 5 cm too short and move their bodies by centimetres in the first
    substep, which the frame's one broadphase (spheres inflated by the START velocities' travel over the frame) cannot foresee:
    pairs that four single-substep frames find in their second broadphase are not in the four-substep frame's lists, and the
    two runs part in substep 2 -- with and without stage 7 alike (finding 3).  That is the broadphase's stated
    contract, not stage 7's, and the figure printed for `chain` is accordingly large."""
    start, _, _, s = dcs.trajectory(name)["frames"][0]
    h = s["h"]
    with xd.new_world() as w:
        fused, single, split = xd.seam_runs(w, lambda: xd.prepare(w, s, start), h)
    state = start
    for _ in range(4):
        res = dcs.model(name, 0, state=state)
        state = xm.native().to_f64(res["state"])
    e = xk.scene_errors(s, fused, res, start)
    print("%s: four substeps against the model chained four times %.1f" % (name, e.max()))
    assert np.abs(fused - start)[:, 31:38].max() > 1e-4
    assert bits_equal(fused, split)
    if not name.startswith("chain"):
        assert bits_equal(fused, single)


def test_velocity_entries_are_reasserted_at_every_substep_and_the_split_api_is_refused():
    """Scene (e) with its VELOCITY entries alone: step(4 h, 4) equals four step(h, 1) bit for bit -- the overwrite at k >= 1 is
    enqueued in another place than the one at k = 0 -- and with a table the split API is XPBD_E_INVALID."""
    start, _, _, s = dcs.trajectory("platforms-h1200")["frames"][0]
    h = s["h"]
    only = s["kinematics"][s["kinematics"]["mode"] == capi.KINEMATIC_VELOCITY]
    assert len(only) == 2
    with xd.new_world() as w:
        fused, single, _ = xd.seam_runs(w, lambda: xd.prepare(w, s, start, kinematics=only), h, split=False)
        xd.prepare(w, s, start, kinematics=only)
        with pytest.raises(capi.XpbdError) as err:
            w.contacts_begin(4 * h)
        assert err.value.code == capi.E_INVALID
    spinner = int(only["body"][1])
    assert np.abs(fused[spinner, 34:38] - start[spinner, 34:38]).max() > 1e-4
    assert bits_equal(fused, single)


def test_a_body_with_the_default_row_has_the_bits_of_the_undamped_world():
    """Body 1 of scene (a) keeps the default row among bodies with rows: after the substep its bits are those of the same world
    stepped without any damping (stage 7 is the substep's last stage and changes nobody else's pose)."""
    t, damped = run("drag-h1200", frames=2)
    _, plain = run("drag-h1200", without=("damping",), frames=2)
    for f in range(2):
        rows = t["frames"][f][3]["rows"]
        dragged = np.nonzero((rows["linear"] > 0) & (rows["angular"] > 0))[0]
        assert len(dragged) >= 10 and not rows[1]["linear"] and not rows[1]["angular"]
        assert bits_equal(damped[f][1], plain[f][1]), f
        differ = (damped[f][dragged, 22:28].view(np.uint64) != plain[f][dragged, 22:28].view(np.uint64)).any(axis=1)
        assert differ.all() and bits_equal(damped[f][:, 31:38], plain[f][:, 31:38]), f


@pytest.mark.parametrize("substeps", dcs.LONE_SUBSTEPS)
def test_lone_pose_entries_arrive_within_the_models_bound(substeps):
    """The 65 lone POSE entries, one frame of S substeps: the end pose against the longdouble model chained S times with
    substeps_left = S - k, within K_LONE[S] -- 8x the f64 evaluation's error against that chain, measured on the CPU."""
    bodies, sid, kin = dcs.lone_scene()
    ref, bad = dcs.lone_chain(substeps)
    with xd.new_world() as w:
        w.upload(bodies, sid)
        w.set_kinematics(kin)
        w.step(dcs.LONE_DT, substeps)
        got = w.download()
    e = np.where(bad, 0.0, dcs.lone_pose_errors(got, ref[-1]))
    print("S = %d: device against the longdouble chain %.4f (K_LONE = %g), body %d" % (substeps, e.max(), dcs.K_LONE[substeps], e.argmax()))
    assert bad.sum() == 1 and np.isfinite(got).all()
    assert e.max() <= dcs.K_LONE[substeps]


def test_a_platform_scene_stepped_with_four_substeps_is_printed_against_the_chained_model():
    """Scene (e), step(4 h, 4) with POSE and VELOCITY entries, against the model chained four times with substeps_left = 4 - k: a
    figure, no bound (the device's rounding of one substep is the next one's input, and a contact may begin one substep apart)."""
    name = "platforms-h1200"
    start, _, _, s = dcs.trajectory(name)["frames"][0]
    h = s["h"]
    with xd.new_world() as w:
        xd.prepare(w, s, start)
        w.step(4 * h, 4)
        got = w.download()
    state = start
    for k in range(4):
        res = dcs.model(name, 0, state=state, substeps_left=4 - k, substep_index=k)
        state = xm.native().to_f64(res["state"])
    e = xk.scene_errors(s, got, res, start)
    print("%s: four substeps against the model chained four times: largest %.3g, median %.3g" % (name, e.max(), np.median(e)))
    assert np.isfinite(got).all()


def test_scene_f_in_a_world_whose_mass_rows_were_edited_in_place():
    """Every body uploaded with the mass row of a unit box; set_mass_properties (INVERSE layout) to the scene's rows, the bodies
    that become kinematic still with mass; those frozen (a zero row, the scene's centre of mass); then set_kinematics.  The step
    has the model's verdict and the bits of the world that uploaded the scene's rows."""
    name = "all-h240"
    t = dcs.trajectory(name)
    unit = pc.new_body(pc.CUBE, (0.0, 0.0, 0.0))
    edited, uploaded = [], []
    with xd.new_world() as w:
        for start, _, _, s in t["frames"]:
            kin = s["kinematics"]["body"].astype(np.int64)
            rows = np.concatenate([start[:, 0:10], start[:, 28:31]], axis=1)
            assert not rows[kin, 0:10].any()
            plain = start.copy()
            plain[:, 0:10], plain[:, 28:31] = unit[0:10], unit[28:31]
            w.upload(plain, s["sid"])
            xd.apply_settings(w, s, without=("kinematics",))
            first = rows.copy()
            first[kin, 0:10] = unit[0:10]
            w.set_mass_properties(None, first, capi.MASS_INVERSE)
            with pytest.raises(capi.XpbdError):                          # a body with mass is refused
                w.set_kinematics(s["kinematics"])
            w.set_mass_properties(kin, rows[kin], capi.MASS_INVERSE)     # freeze
            w.set_kinematics(s["kinematics"])
            assert np.array_equal(w.get_mass_properties(), rows)
            w.step(s["h"], 1)
            edited.append(w.download())
            xd.prepare(w, s, start)
            w.step(s["h"], 1)
            uploaded.append(w.download())
    xd.verdict(dcs, name, edited)
    for f in range(len(edited)):
        assert bits_equal(edited[f], uploaded[f]), f
