"""Damping on the GPU (include/xpbd.h, "DAMPING"): body drag, speed caps and joint dampers, stage 7 of every substep.

Expected frames are the committed oracle's, run one substep at a time with the model's stage 7 (tests/damping_model.py) applied
after each -- with restitution on, the restitution model's stage 6 in between; tests/test_damping_model.py shows that yardstick
valid on these scenes.  The pass uses only + - * / and sqrt, which are correctly rounded on the device, so every body must
equal the expected frame bit for bit.

Shapes: 16 to 32 unit boxes, 8 substeps, 3 or 4 frames (damping_common.py); the physical tests run the frames they need."""

import numpy as np
import pytest

import damping_common as dc
import damping_model as dm
import kinematic_common as kc
import kinematic_model as km
import sleep_common as sc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu


def differing(got, want):
    return np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))


# ---- 1. off is off ----------------------------------------------------------------------------------------------------------
def test_defaults_and_reset_values_step_like_a_world_that_never_called_the_setters():
    bodies, sid, joints, rows, dampers, _ = dc.scene("chain_on_pile")
    n = len(bodies)

    def run(prepare):
        with dc.new_world(bodies, sid, joints) as w:
            prepare(w)
            out = []
            for _ in range(dc.FRAMES):
                w.step(dc.DT, dc.SUBSTEPS)
                out.append(w.download())
            return out

    def defaults(w):
        w.set_damping(capi.body_damping(n))
        w.set_joint_damping(None)
        w.set_joint_damping(capi.joint_damping(np.arange(len(joints)), 0.0, 0.0))     # listed, every coefficient zero

    def set_and_reset(w):
        w.set_damping(rows)
        w.set_joint_damping(dampers)
        w.step(dc.DT, dc.SUBSTEPS)                                    # the pass has run ...
        w.upload(bodies, sid)                                         # ... and the scene starts again
        w.set_joints(joints)
        w.set_damping(rows)
        w.set_joint_damping(dampers)
        w.set_damping(None)
        w.set_joint_damping(None)

    never = run(lambda w: None)
    for name, prepare in (("defaults", defaults), ("reset", set_and_reset)):
        got = run(prepare)
        for f in range(dc.FRAMES):
            assert bits_equal(got[f], never[f]), (name, f, differing(got[f], never[f]))
    plain = dc.expected("chain_on_pile", damped=False)
    assert bits_equal(never[-1], plain[-1])                           # and that world is the oracle's


# ---- 2. GPU == model, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES)
def test_the_world_equals_the_model_bit_for_bit(name):
    want, got = dc.expected(name), dc.run_world(name)
    for f in range(dc.FRAMES):
        assert bits_equal(got[f], want[f]), (name, f, differing(got[f], want[f]))
    assert not bits_equal(got[-1], dc.expected(name, damped=False)[-1])


def test_the_world_equals_the_model_under_gjk_epa():
    want, got = dc.expected("chain_on_pile", narrowphase=1), dc.run_world("chain_on_pile", capi.NARROWPHASE_GJK_EPA)
    for f in range(dc.FRAMES):
        assert bits_equal(got[f], want[f]), (f, differing(got[f], want[f]))


def test_the_split_api_runs_the_pass_as_the_step_does():
    bodies, sid, joints, rows, dampers, _ = dc.scene("chain_on_pile")
    want = dc.expected("chain_on_pile")
    with dc.new_world(bodies, sid, joints) as w:
        w.set_damping(rows)
        w.set_joint_damping(dampers)
        for f in range(2):
            w.contacts_begin(dc.DT)
            for _ in range(dc.SUBSTEPS):
                w.contacts_substep(dc.H)
            assert bits_equal(w.download(), want[f]), f


# ---- 3. caps hold -----------------------------------------------------------------------------------------------------------
def squeeze_run(caps):
    bodies, sid = dc.squeeze_scene()
    out = []
    with dc.new_world(bodies, sid) as w:
        if caps:
            w.set_damping(capi.body_damping(len(bodies), max_linear_speed=dc.CAP_LINEAR, max_angular_speed=dc.CAP_ANGULAR))
        for _ in range(dc.SQUEEZE_FRAMES):
            w.step(dc.DT, dc.SUBSTEPS)
            out.append(w.download())
    return out


def test_caps_hold_after_every_frame_and_the_uncapped_scene_exceeds_them():
    free, capped = squeeze_run(False), squeeze_run(True)
    lin = np.array([dc.speeds(f)[0] for f in free])
    ang = np.array([dc.speeds(f)[1] for f in free])
    print("uncapped: largest speed %.3f m/s, %.3f rad/s" % (lin.max(), ang.max()))
    assert lin.max() > dc.CAP_LINEAR and ang.max() > dc.CAP_ANGULAR   # not vacuous: the same scene without caps exceeds both
    hit_linear = hit_angular = False
    for f, rows in enumerate(capped):
        lin, ang = dc.speeds(rows)
        # the issue's bound, two roundings per component; the norm itself is formed here with a few more
        assert np.all(np.sqrt((rows[:, 22:25] ** 2).sum(axis=1)) <= dc.CAP_LINEAR * (1.0 + 1e-15)), (f, lin)
        assert np.all(np.sqrt((rows[:, 25:28] ** 2).sum(axis=1)) <= dc.CAP_ANGULAR * (1.0 + 1e-15)), (f, ang)
        hit_linear |= bool(np.any(lin > dc.CAP_LINEAR * (1.0 - 1e-12)))
        hit_angular |= bool(np.any(ang > dc.CAP_ANGULAR * (1.0 - 1e-12)))
    assert hit_linear and hit_angular                                 # and both caps were what held a body


# ---- 4. a damper damps ------------------------------------------------------------------------------------------------------
def pendulum_run(mu_a, seconds=dc.PENDULUM_SECONDS):
    """(angle_rate after every frame, largest |w_b - w_a| component after any frame)."""
    bodies, sid, joints, limits = dc.pendulum_scene()
    rates, relative = [], 0.0
    with dc.new_world(bodies, sid, joints) as w:
        w.set_joint_limits(limits)
        if mu_a:
            w.set_joint_damping(capi.joint_damping([0], 0.0, mu_a))
        for _ in range(60 * seconds):
            w.step(dc.DT, dc.SUBSTEPS)
            state = w.joint_states()[0]
            assert state["flags"] & capi.JOINT_STATE_HAS_ANGLE
            rates.append(float(state["angle_rate"]))
            rows = w.download()
            relative = max(relative, float(np.abs(rows[1, 25:28] - rows[0, 25:28]).max()))
    return rates, relative


def test_a_joint_damper_makes_every_swing_smaller_and_a_stiff_one_stops_the_relative_spin():
    mu = 10.0
    assert mu * dc.H < 1.0
    free, _ = pendulum_run(0.0)
    damped, _ = pendulum_run(mu)
    peaks = dc.swing_peaks(damped)
    print("peaks of the damped swings:", ["%.4f" % p for p in peaks], "undamped:", ["%.4f" % p for p in dc.swing_peaks(free)])
    assert len(peaks) >= 3 and all(b < a for a, b in zip(peaks, peaks[1:])), peaks
    assert max(abs(r) for r in damped[-60:]) < max(abs(r) for r in free[-60:])
    # mu_a h >= 1 on an isotropic box from a fixed body: the damper removes the whole relative angular velocity in every substep.
    # (The issue's bound is 1e-12 * (1 + |w| before); |w| before cannot be seen from outside, so the bound is taken at |w| = 0.)
    _, relative = pendulum_run(1.0 / dc.H, seconds=1)
    print("largest |w_b - w_a| with mu_a h = 1: %.3e" % relative)
    assert relative <= 1e-12


# ---- 5. kinematic and fixed bodies ignore it ---------------------------------------------------------------------------------
def test_a_conveyor_with_a_drag_row_keeps_its_speed_and_its_rider_is_dragged():
    bodies, sid, tbl = kc.velocity_scene()
    rows = dm.rows(len(bodies), linear=5.0, angular=5.0, max_linear_speed=0.05, max_angular_speed=0.05)
    h = kc.DT / kc.VELOCITY_SUBSTEPS

    def run(damped):
        with kc.new_world(bodies, sid) as w:
            w.set_kinematics(kc.to_capi(tbl))
            if damped:
                w.set_damping(rows)
            out = []
            for _ in range(kc.VELOCITY_FRAMES):
                w.step(kc.DT, kc.VELOCITY_SUBSTEPS)
                out.append(w.download())
            return out

    free, damped = run(False), run(True)
    b = bodies
    for f in range(kc.VELOCITY_FRAMES):
        for k in range(kc.VELOCITY_SUBSTEPS):                        # the model: overwrite, the oracle's substep, stage 7
            b, _ = km.overwrite(b, tbl, h, kc.VELOCITY_SUBSTEPS - k)
            b = dm.oracle_substeps(b, sid, kc.polys(), kc.NO_JOINTS, h, 1, kc.PAD, rows)
        assert bits_equal(damped[f], b), (f, differing(damped[f], b))
        for i in (kc.CONVEYOR, kc.TURNTABLE, kc.BOTH):               # scripted bodies: the undamped world's bits, capped row or not
            assert bits_equal(damped[f][i], free[f][i]), (f, i)
    assert np.linalg.norm(damped[-1][kc.CONVEYOR, 22:25]) > 0.3      # far above its row's cap
    assert np.linalg.norm(damped[-1][kc.RIDER, 22:25]) <= 0.05 * (1.0 + 1e-15) < np.linalg.norm(free[-1][kc.RIDER, 22:25])


# ---- 6. lifetimes -----------------------------------------------------------------------------------------------------------
def test_rows_and_dampers_follow_a_population_change_and_the_setters_that_clear_them():
    bodies, sid, joints, rows, dampers, _ = dc.scene("chain_on_pile")
    n = len(bodies)
    gone = [2, dc.N_PILE + 3]                                         # a box of the pile, and the chain's third link with joints 2 and 3
    keep = [i for i in range(n) if i not in gone]
    newcomers, new_sid = kc.boxes(2, [[8.0, 8.0, 0.5], [8.0, 8.0, 1.6]])
    with dc.new_world(bodies, sid, joints) as w:
        assert w.get_damping().tobytes() == capi.body_damping(n).tobytes()
        w.set_damping(rows)
        w.set_joint_damping(dampers)
        assert w.get_damping().tobytes() == rows.tobytes()
        w.step(dc.DT, dc.SUBSTEPS)
        old_to_new, joint_map = w.remove_bodies(gone)
        assert w.get_damping().tobytes() == rows[keep].tobytes()
        w.add_bodies(newcomers, new_sid)
        want_rows = np.concatenate([rows[keep], capi.body_damping(2)])
        assert w.get_damping().tobytes() == want_rows.tobytes()
        state = w.download()
        changed = []
        for _ in range(2):
            w.step(dc.DT, dc.SUBSTEPS)
            changed.append(w.download())
    # a fresh world given the download, the re-indexed joints, the rows and the re-indexed dampers
    kept_joints = joints[joint_map != capi.NO_HIT].copy()
    kept_joints["body_a"], kept_joints["body_b"] = old_to_new[kept_joints["body_a"]], old_to_new[kept_joints["body_b"]]
    kept_dampers = dampers[joint_map[dampers["joint"]] != capi.NO_HIT].copy()
    kept_dampers["joint"] = joint_map[kept_dampers["joint"]]
    assert len(kept_joints) == len(joints) - 2 and 0 < len(kept_dampers) < len(dampers)
    with dc.new_world(state, np.zeros(len(state), dtype=np.uint32), kept_joints) as w:
        w.set_damping(want_rows)
        w.set_joint_damping(kept_dampers.view(capi.JOINT_DAMPING_DTYPE))
        for f in range(2):
            w.step(dc.DT, dc.SUBSTEPS)
            assert bits_equal(w.download(), changed[f]), (f, differing(w.download(), changed[f]))

    # who clears what: the run after each call equals the run of a world that holds exactly what should be left
    def frames_after(prepare):
        with dc.new_world(bodies, sid, joints) as w:
            prepare(w)
            out, in_force = [], w.get_damping()
            for _ in range(2):
                w.step(dc.DT, dc.SUBSTEPS)
                out.append(w.download())
            return out, in_force

    def both(w):
        w.set_damping(rows)
        w.set_joint_damping(dampers)

    def rows_only(w):
        w.set_damping(rows)

    def set_joints_again(w):
        both(w)
        w.set_joints(joints)                                          # clears the dampers, not the rows

    def limits_and_targets(w):
        both(w)
        w.set_joint_limits(np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE))  # neither clears anything
        w.set_joint_drives(np.zeros(0, dtype=capi.JOINT_DRIVE_DTYPE))
        w.set_drive_targets(None, np.zeros(0))

    def upload_again(w):
        both(w)
        w.upload(bodies, sid)                                         # clears both (and the joints)
        w.set_joints(joints)

    full, full_rows = frames_after(both)
    for prepare, (want, want_rows) in ((set_joints_again, frames_after(rows_only)), (limits_and_targets, (full, full_rows)),
                                       (upload_again, frames_after(lambda w: None))):
        got, got_rows = frames_after(prepare)
        assert got_rows.tobytes() == want_rows.tobytes(), prepare.__name__
        for f in range(2):
            assert bits_equal(got[f], want[f]), (prepare.__name__, f)
    assert not bits_equal(full[-1], frames_after(rows_only)[0][-1])   # the dampers matter in this scene


def test_refusals_leave_the_previous_values_in_force():
    bodies, sid, joints, rows, dampers, _ = dc.scene("chain_on_pile")
    n = len(bodies)
    want = dc.expected("chain_on_pile")
    L = capi.hip_lib()
    with dc.new_world(bodies, sid, joints) as w:
        w.set_damping(rows)
        w.set_joint_damping(dampers)
        bad = rows.copy()
        bad["linear"][3] = -1.0
        twice = capi.joint_damping([1, 1], 1.0, 1.0)
        for call, args, word in ((L.xpbd_world_set_damping, (bad.ctypes.data, n), b"rows[3].linear"),
                                 (L.xpbd_world_set_damping, (rows.ctypes.data, n - 1), b"bodies"),
                                 (L.xpbd_world_set_damping, (None, n), b"NULL rows"),
                                 (L.xpbd_world_get_damping, (bad.ctypes.data, n + 1), b"bodies"),
                                 (L.xpbd_world_set_joint_damping, (twice.ctypes.data, 2), b"second entry"),
                                 (L.xpbd_world_set_joint_damping, (capi.joint_damping([len(joints)], 1.0, 0.0).ctypes.data, 1), b"names joint"),
                                 (L.xpbd_world_set_joint_damping, (None, 1), b"NULL list")):
            assert call(w._h, *args) == capi.E_INVALID
            assert word in L.xpbd_last_error(), (word, L.xpbd_last_error())
        assert w.get_damping().tobytes() == rows.tobytes()
        w.step(dc.DT, dc.SUBSTEPS)
        assert bits_equal(w.download(), want[0])
    for mode in (capi.MODE_FUSED, capi.MODE_PER_SUBSTEP):             # the pinned modes: rows accepted and ignored, dampers refused
        verts, off = capi.scene_shapes(capi.SCENE_BOXES)
        with capi.World(mode=mode) as w:
            w.set_shapes(verts, off)
            w.upload(bodies, sid)
            w.step(dc.DT, dc.SUBSTEPS)
            before = w.download()
            w.upload(bodies, sid)
            w.set_damping(rows)
            w.step(dc.DT, dc.SUBSTEPS)
            assert bits_equal(w.download(), before), mode
            one = capi.joint_damping([0], 1.0, 0.0)
            assert L.xpbd_world_set_joint_damping(w._h, one.ctypes.data, 1) == capi.E_INVALID and b"XPBD_MODE_CONTACTS" in L.xpbd_last_error()
            w.set_joint_damping(None)                                 # clearing nothing is accepted


# ---- 7. sleeping ------------------------------------------------------------------------------------------------------------
FIXED_BOX = 5                  # appended to the stack scene: sleepers, a FIXED body and an awake one (FALLING) share a wave


def sleeping_run(drag):
    bodies, sid = sc.stack_scene()
    slab, slab_sid = kc.boxes(1, [[60.0, 0.0, 3.0]], fixed=[0])
    bodies, sid = np.concatenate([bodies, slab]), np.concatenate([sid, slab_sid])
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
    w.upload(bodies, sid)
    w.set_contact_report(True)
    w.set_sleeping(*dc.SLEEP_CFG)
    if drag:
        w.set_damping(capi.body_damping(len(bodies), linear=drag, angular=drag))
    with w:
        frames, _ = sc.run_against_model(w, sc.ic.distance_joints([], []), dc.SLEEP_CFG, dc.SLEEP_FRAMES, substeps=dc.SLEEP_SUBSTEPS)
    return bodies, sid, frames


def test_the_cycling_stack_sleeps_with_drag_and_not_without():
    _, _, free = sleeping_run(0.0)
    assert not any(f.asleep[list(sc.STACK)].any() for f in free)      # thresholds below its jitter: it never rests
    bodies, sid, damped = sleeping_run(dc.SLEEP_DRAG)
    first = next((k for k, f in enumerate(damped) if f.asleep[list(sc.STACK)].all()), None)
    print("the stack sleeps after frame %s of %d (model: calm from frame %d)" % (None if first is None else first + 1, dc.SLEEP_FRAMES, dc.SLEEP_MODEL_FRAME))
    assert first is not None and damped[-1].asleep[list(sc.STACK)].all()
    assert sc.assert_frozen(damped) > 0                               # a sleeper stays bit-frozen under the pass
    assert not damped[-1].asleep[sc.FALLING] and not damped[-1].asleep[FIXED_BOX]
    # the awake body in the sleepers' wave is the model's, bit for bit (it is alone out there), and the fixed one is untouched
    alone = bodies[[sc.FALLING]]
    rows = dm.rows(1, linear=dc.SLEEP_DRAG, angular=dc.SLEEP_DRAG)
    for k, f in enumerate(damped):
        alone = dm.oracle_substeps(alone, sid[:1], dc.polys(), dc.NO_JOINTS, dc.DT, dc.SLEEP_SUBSTEPS, dc.PAD, rows)
        assert bits_equal(f.bodies[sc.FALLING], alone[0]), k
        assert bits_equal(f.bodies[FIXED_BOX], bodies[FIXED_BOX]), k
