"""Sliders, SLIDE limits and joint drives (xpbd_world_set_joint_drives, xpbd_multi_world_set_joint_drives) on the GPU: the
device agrees with the independent model (tests/joint_drive_model.py), the eight-lane and the one-lane pair solve give the
same bits, clearing restores every bit, the known-answer scenes of tests/test_joint_drive_model.py behave on the device as
in the model, a sharded world equals the single one bit for bit, history restore reproduces a run, and bad arguments are
rejected with the previous drives left in place."""
import math

import numpy as np
import pytest

import joint_drive_model as jd
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import line_scene

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
X, Y, Z = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
INF = float("inf")
NO_LIMITS = np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE)
NO_DRIVES = np.zeros(0, dtype=capi.JOINT_DRIVE_DTYPE)


def limits(*rows):
    """rows of (joint, kind, lower, upper[, ref_a, ref_b])"""
    out = np.zeros(len(rows), dtype=capi.JOINT_LIMIT_DTYPE)
    for k, r in enumerate(rows):
        out[k]["joint"], out[k]["kind"], out[k]["lower"], out[k]["upper"] = r[:4]
        out[k]["ref_a"], out[k]["ref_b"] = (r[4], r[5]) if len(r) > 4 else (X, X)
    return out


def drives(*rows):
    """rows of (joint, kind, target[, compliance, max_force, ref_a, ref_b])"""
    out = np.zeros(len(rows), dtype=capi.JOINT_DRIVE_DTYPE)
    for k, r in enumerate(rows):
        out[k]["joint"], out[k]["kind"], out[k]["target"] = r[:3]
        out[k]["compliance"] = r[3] if len(r) > 3 else 0.0
        out[k]["max_force"] = r[4] if len(r) > 4 else INF
        out[k]["ref_a"], out[k]["ref_b"] = (r[5], r[6]) if len(r) > 5 else (X, X)
    return out


def run_world(kind, bodies, sid, joints, lims, drvs, frames, substeps, dt=DT, every=False):
    out = []
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies, sid)
        w.set_joints(joints)
        if lims is not None:
            w.set_joint_limits(lims)
        if drvs is not None:
            w.set_joint_drives(drvs)
        for _ in range(frames):
            w.step(dt, substeps)
            if every:
                out.append(w.download())
        return out if every else w.download()


# ---- 1. the device agrees with the model ------------------------------------------------------------------------------
def random_driven_scene(seed, n_bodies=6):
    """Free cubes in a row 2 m apart (their bounding spheres never meet), tilted and spinning, no gravity, as the scenes of
    tests/test_gpu_joint_limits.py; hinges and sliders between neighbours with hinge limits, SLIDE limits and drives of all four
    kinds, some soft and some with a finite max_force, listed in a shuffled order."""
    rng = np.random.default_rng(2000 + seed)
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, n_bodies)
    bodies[:, 10:22] = 0.0
    lim_rows, drv_rows = [], []
    joints = np.zeros(n_bodies - 1, dtype=capi.JOINT_DTYPE)
    for i in range(n_bodies):
        axis = rng.normal(size=3)
        angle = rng.uniform(-0.3, 0.3)
        bodies[i, 31:34] = [2.0 * i, 0.0, 3.0]
        bodies[i, 34:38] = np.concatenate([[math.cos(angle / 2)], axis / np.linalg.norm(axis) * math.sin(angle / 2)])
        bodies[i, 22:25] = rng.normal(scale=0.3, size=3)
        bodies[i, 25:28] = rng.normal(scale=4.0, size=3)
    if seed % 2:
        bodies[0, 0:10] = 0.0                                           # a static end
    for k in range(n_bodies - 1):
        j = joints[k]
        j["body_a"], j["body_b"] = k, k + 1
        j["anchor_a"], j["anchor_b"] = [1.5, 0.5, 0.5], [-0.5, 0.5, 0.5]
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ref = np.cross(axis, rng.normal(size=3))
        ref /= np.linalg.norm(ref)
        j["axis_a"] = j["axis_b"] = axis
        soft = rng.uniform(0.0, 0.01) if rng.uniform() < 0.5 else 0.0
        weak = rng.uniform(0.5, 5.0) if rng.uniform() < 0.5 else INF
        slider = rng.uniform() < 0.5
        j["kind"] = capi.JOINT_SLIDER if slider else capi.JOINT_HINGE
        if rng.uniform() < 0.4:
            lo = rng.uniform(-0.2, 0.0)
            lim_rows.append((k, capi.LIMIT_HINGE, lo, lo + rng.uniform(0.0, 0.2), ref, ref))
        if rng.uniform() < (0.5 if slider else 0.9):
            if rng.uniform() < 0.5:
                drv_rows.append((k, capi.DRIVE_ANGLE, rng.uniform(-0.3, 0.3), soft, weak, ref, ref))
            else:
                drv_rows.append((k, capi.DRIVE_ANGULAR_VELOCITY, rng.uniform(-5.0, 5.0), soft, weak, ref, ref))
        if slider:
            if rng.uniform() < 0.6:
                lo = rng.uniform(-0.05, 0.0)
                lim_rows.append((k, capi.LIMIT_SLIDE, lo, lo + rng.uniform(0.0, 0.05)))
            if rng.uniform() < 0.8:
                soft = rng.uniform(0.0, 0.01) if rng.uniform() < 0.5 else 0.0
                weak = rng.uniform(0.5, 5.0) if rng.uniform() < 0.5 else INF
                if rng.uniform() < 0.5:
                    drv_rows.append((k, capi.DRIVE_POSITION, rng.uniform(-0.2, 0.2), soft, weak))
                else:
                    drv_rows.append((k, capi.DRIVE_VELOCITY, rng.uniform(-2.0, 2.0), soft, weak))
    lim_rows = [lim_rows[i] for i in rng.permutation(len(lim_rows))]    # the caller's order need not be the joints'
    drv_rows = [drv_rows[i] for i in rng.permutation(len(drv_rows))]
    return bodies, sid, joints, limits(*lim_rows), drives(*drv_rows)


def without_extras(lims):
    return lims[lims["kind"] != capi.LIMIT_SLIDE]


def test_device_matches_the_model_on_random_driven_joints():
    worst, differs, kinds = 0.0, 0, set()
    for seed in range(30):
        bodies, sid, joints, lims, drvs = random_driven_scene(seed)
        kinds |= set(drvs["kind"].tolist()) | {10 + k for k in lims["kind"].tolist()} | {20 + k for k in joints["kind"].tolist()}
        want = jd.step(bodies, joints, lims, drvs, DT, 20)
        plain = jd.step(bodies, joints, without_extras(lims), NO_DRIVES, DT, 20)
        differs += np.abs(plain - want).max() > 1e-6                   # the drives and SLIDE limits acted
        got = run_world(capi.SCENE_BOXES, bodies, sid, joints, lims, drvs, 1, 20)
        worst = max(worst, np.abs(got - want).max())
        print("seed %d: largest |GPU - model| %.3g" % (seed, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10, err_msg="seed %d" % seed)
    assert differs >= 25, differs
    assert kinds >= {0, 1, 2, 3, 10 + capi.LIMIT_HINGE, 10 + capi.LIMIT_SLIDE, 20 + capi.JOINT_HINGE, 20 + capi.JOINT_SLIDER}
    print("largest |GPU - model| over 30 scenes: %.3g" % worst)


# ---- 2. eight lanes per body == one lane per body ---------------------------------------------------------------------
def test_small_world_path_equals_large_world_path():
    bodies, sid, joints, lims, drvs = random_driven_scene(3)
    alone = run_world(capi.SCENE_BOXES, bodies, sid, joints, lims, drvs, 1, 20)
    n_fill = SMALL_WORLD + 64 - len(bodies)
    fill, fill_sid = capi.scene_generate(capi.SCENE_BOXES, 2, n_fill)
    fill[:, 10:28] = 0.0
    fill[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    side = int(math.ceil(math.sqrt(n_fill)))
    fill[:, 31] = 100.0 + 3.0 * (np.arange(n_fill) % side)              # a resting grid far away, 3 m pitch, above the ground
    fill[:, 32] = 100.0 + 3.0 * (np.arange(n_fill) // side)
    fill[:, 33] = 3.0
    big = run_world(capi.SCENE_BOXES, np.concatenate([bodies, fill]), np.concatenate([sid, fill_sid]), joints, lims, drvs, 1, 20)
    assert bits_equal(big[:len(bodies)], alone)
    assert bits_equal(big[len(bodies):, 31:38], fill[:, 31:38])         # (the fillers stayed where they were)


# ---- 3. clearing ----------------------------------------------------------------------------------------------------
def test_clearing_drives_restores_every_bit():
    bodies, sid, joints, lims, drvs = random_driven_scene(4)
    assert len(drvs) and len(lims)
    never = run_world(capi.SCENE_BOXES, bodies, sid, joints, lims, None, 2, 20)
    driven = run_world(capi.SCENE_BOXES, bodies, sid, joints, lims, drvs, 2, 20)
    assert not bits_equal(driven, never)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        for clear in ("empty", "set_joints", "upload", "set_joint_limits keeps them"):
            w.upload(bodies, sid)
            w.set_joints(joints)
            w.set_joint_limits(lims)
            w.set_joint_drives(drvs)
            if clear == "empty":
                w.set_joint_drives(NO_DRIVES)
            elif clear == "set_joints":
                w.set_joints(joints)
                w.set_joint_limits(lims)
            elif clear == "upload":
                w.upload(bodies, sid)
                w.set_joints(joints)
                w.set_joint_limits(lims)
            else:
                w.set_joint_limits(NO_LIMITS)
                w.set_joint_limits(lims)                                # limits and drives do not clear each other
            for _ in range(2):
                w.step(DT, 20)
            assert bits_equal(w.download(), driven if clear.startswith("set_joint_limits") else never), clear
        w.upload(bodies, sid)                                           # ... nor do the drives clear the limits
        w.set_joints(joints)
        w.set_joint_limits(lims)
        w.set_joint_drives(drvs)
        w.set_joint_drives(NO_DRIVES)
        w.set_joint_drives(drvs)
        for _ in range(2):
            w.step(DT, 20)
        assert bits_equal(w.download(), driven)


# ---- 4. behaviour -----------------------------------------------------------------------------------------------------
def device_stepper(rows, joints, lims, drvs, steps, substeps, dt):
    sid = np.zeros(len(rows), dtype=np.uint32)
    return run_world(capi.SCENE_BOXES, rows, sid, joints.astype(capi.JOINT_DTYPE), lims.astype(capi.JOINT_LIMIT_DTYPE),
                     drvs.astype(capi.JOINT_DRIVE_DTYPE), steps, substeps, dt, every=True)


_PATHS = {}


def both_paths(scene):
    if scene not in _PATHS:
        _PATHS[scene] = (jd.run_scene(scene), jd.run_scene(scene, device_stepper))
    return _PATHS[scene]


# The figure of every known-answer scene on the device is held to the known answer, with twice the model's own deviation from
# it as margin (the model's deviations are explained, bound by bound, in tests/test_joint_drive_model.py).  Where that
# deviation is rounding noise, the margin is no less than what the device may differ from the model by anyway: 1e-10 on a pose
# (the bound of the first test), and on a velocity an ulp of the position per substep taken through derive's 1 / h.
H20 = DT / 20
VELOCITY_NOISE = 600 * np.spacing(26.0) / H20


@pytest.mark.parametrize("figure,floor", [("wheel", 2e-10 / DT), ("spring", 1e-10), ("incline", VELOCITY_NOISE), ("incline_perpendicular", 1e-10),
                                          ("incline_stop", 1e-10), ("lift_weak", VELOCITY_NOISE), ("lift_strong", VELOCITY_NOISE),
                                          ("prismatic", 1e-10)])
def test_known_answers_hold_on_the_device(figure, floor):
    model_path, device_path = both_paths(jd.FIGURES[figure])
    model, answer = jd.measure(figure, model_path)
    device, _ = jd.measure(figure, device_path)
    margin = max(2 * abs(model - answer), floor)
    print("%s: known answer %.17g, model %.17g, device %.17g, margin %.3g" % (figure, answer, model, device, margin))
    assert abs(device - answer) <= margin


def test_controls_without_stop_and_without_lock_move_on():
    """The SLIDE limit and the hinge limit 0/0 of the scenes above are what holds the body: without them it goes on."""
    slid, free_fall = jd.measure("incline_free", both_paths("incline_free")[1])
    assert slid > 1.9 * jd.SLIDE_STOP and abs(slid - free_fall) < 2e-3
    turned, _ = jd.measure("cylindrical", both_paths("cylindrical")[1])
    assert turned > 0.99


# ---- 5. sharded == single ---------------------------------------------------------------------------------------------
def driven_chain(n):
    """A two-row line of dropped boxes (contacts with the ground and each other); the first row is one chain, every box linked
    to the next by a hinge or a slider about y, each with a drive: wherever the row is cut, a driven joint crosses the cut."""
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    joints = np.zeros(n // 2 - 1, dtype=capi.JOINT_DTYPE)
    joints["body_a"] = np.arange(n // 2 - 1)
    joints["body_b"] = joints["body_a"] + 1
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    joints["axis_a"] = joints["axis_b"] = Y
    sliders = np.arange(len(joints)) % 2 == 1
    joints["kind"] = np.where(sliders, capi.JOINT_SLIDER, capi.JOINT_HINGE)
    lim_rows, drv_rows = [], []
    for k in range(len(joints)):
        if sliders[k]:
            lim_rows += [(k, capi.LIMIT_SLIDE, -0.05, 0.05), (k, capi.LIMIT_HINGE, -0.3, 0.3)]
            drv_rows.append((k, capi.DRIVE_VELOCITY, 0.5 if k % 4 == 1 else -0.5, 0.0, 40.0))
            if k % 4 == 1:
                drv_rows.append((k, capi.DRIVE_ANGLE, 0.1, 0.001, INF))
        else:
            drv_rows.append((k, capi.DRIVE_ANGULAR_VELOCITY, 2.0, 0.0, 30.0) if k % 4 == 0 else (k, capi.DRIVE_ANGLE, -0.2, 0.002, INF))
    return kind, bodies, sid, joints, limits(*lim_rows), drives(*drv_rows[::-1])


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_sharded_world_with_driven_joints_across_cuts_equals_single(n_ranks):
    n, substeps, frames = 96, 6, 25
    kind, bodies, sid, joints, lims, drvs = driven_chain(n)
    one = run_world(kind, bodies, sid, joints, lims, drvs, frames, substeps)
    assert not bits_equal(one, run_world(kind, bodies, sid, joints, lims, None, frames, substeps))
    with capi.World(mode=capi.MODE_CONTACTS) as w:                      # contacts are present
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies, sid)
        w.set_joints(joints)
        w.set_joint_limits(lims)
        w.set_joint_drives(drvs)
        for _ in range(frames):
            w.step(DT, substeps)
        assert w.contact_stats()[0] > 0
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        mw.set_joint_limits(lims)
        mw.set_joint_drives(drvs)                                       # before the first step: the plan hands them to the shards
        owner = mw.owners()
        for _ in range(frames):
            mw.step(DT, substeps)
        got = mw.download()
    crossing = owner[joints["body_a"]] != owner[joints["body_b"]]
    assert crossing.any()
    assert not np.isnan(one).any() and bits_equal(got, one)


# ---- 6. history -------------------------------------------------------------------------------------------------------
def test_history_restore_reproduces_a_driven_run():
    """The velocity drives keep no state beyond the bodies': a restored world steps to the same bits."""
    bodies, sid, joints, lims, _ = random_driven_scene(5)               # (sliders and hinges, a static end)
    rows = []
    for k, j in enumerate(joints):
        ref = jd.perpendicular_to(j["axis_a"])
        rows.append((k, capi.DRIVE_ANGULAR_VELOCITY, 2.0 - k, 0.0, INF, ref, ref))
        if j["kind"] == capi.JOINT_SLIDER:
            rows.append((k, capi.DRIVE_VELOCITY, 0.5 * (k - 2), 0.001, 8.0))
    drvs = drives(*rows)
    assert (drvs["kind"] == capi.DRIVE_VELOCITY).any()
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        w.set_joints(joints)
        w.set_joint_limits(lims)
        w.set_joint_drives(drvs)
        w.step(DT, 20)
        index = w.history_push()
        for _ in range(3):
            w.step(DT, 20)
        first = w.download()
        w.history_restore(index)
        for _ in range(3):
            w.step(DT, 20)
        assert bits_equal(w.download(), first)
        w.set_joint_drives(NO_DRIVES)                                   # (and the drives did act)
        w.history_restore(index)
        for _ in range(3):
            w.step(DT, 20)
        assert not bits_equal(w.download(), first)


# ---- 7. errors --------------------------------------------------------------------------------------------------------
def mechanism():
    """A hinged wheel (joint 0, axis z), a slider (joint 1, axis x) and a ball joint (joint 2) on three static posts."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 6)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 10:28] = 0.0
    for k, p in enumerate([[0, 0, 5], [2.5, 0, 5], [0, 6, 5], [2.5, 6, 5], [0, 12, 5], [2.5, 12, 5]]):
        bodies[k, 31:34] = p
    bodies[[0, 2, 4], 0:10] = 0.0
    joints = np.zeros(3, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = [0, 2, 4], [1, 3, 5]
    joints["anchor_a"], joints["anchor_b"] = [2.0, 0.0, 0.5], [-0.5, 0.0, 0.5]
    joints["axis_a"][0] = joints["axis_b"][0] = Z
    joints["axis_a"][1:] = joints["axis_b"][1:] = X
    joints["kind"] = [capi.JOINT_HINGE, capi.JOINT_SLIDER, capi.JOINT_DISTANCE]
    good = drives((0, capi.DRIVE_ANGULAR_VELOCITY, 3.0, 0.0, INF, X, X), (1, capi.DRIVE_VELOCITY, 0.5, 0.0, INF),
                  (1, capi.DRIVE_ANGLE, 0.3, 0.01, INF, Y, Y))
    return bodies, sid, joints, good


def bad_drive_cases():
    """(name, drives) that xpbd_world_set_joint_drives must reject for the joints of mechanism()"""
    spin = (0, capi.DRIVE_ANGULAR_VELOCITY, 3.0, 0.0, INF, X, X)
    push = (1, capi.DRIVE_VELOCITY, 0.5, 0.0, INF)
    nan = float("nan")
    return {
        "joint out of range": drives((3, capi.DRIVE_ANGLE, 0.1, 0.0, INF, X, X)),
        "unknown kind": drives((0, 4, 0.1, 0.0, INF, X, X)),
        "angular drive on a ball joint": drives((2, capi.DRIVE_ANGLE, 0.1, 0.0, INF, Y, Y)),
        "linear drive on a hinge": drives((0, capi.DRIVE_POSITION, 0.1)),
        "velocity drive on a ball joint": drives((2, capi.DRIVE_VELOCITY, 0.1)),
        "two angular drives": drives(spin, (0, capi.DRIVE_ANGLE, 0.1, 0.0, INF, X, X)),
        "two linear drives": drives(push, (1, capi.DRIVE_POSITION, 0.1)),
        "non-unit reference": drives((0, capi.DRIVE_ANGLE, 0.1, 0.0, INF, [2.0, 0.0, 0.0], X)),
        "reference along the axis": drives((0, capi.DRIVE_ANGLE, 0.1, 0.0, INF, X, Z)),
        "NaN target": drives((0, capi.DRIVE_ANGULAR_VELOCITY, nan, 0.0, INF, X, X)),
        "infinite target": drives((1, capi.DRIVE_POSITION, INF)),
        "angle target beyond pi": drives((0, capi.DRIVE_ANGLE, 3.2, 0.0, INF, X, X)),
        "negative compliance": drives((1, capi.DRIVE_VELOCITY, 0.5, -1e-3, INF)),
        "infinite compliance": drives((1, capi.DRIVE_VELOCITY, 0.5, INF, INF)),
        "NaN compliance": drives((1, capi.DRIVE_VELOCITY, 0.5, nan, INF)),
        "max_force zero": drives((1, capi.DRIVE_VELOCITY, 0.5, 0.0, 0.0)),
        "max_force negative": drives((1, capi.DRIVE_VELOCITY, 0.5, 0.0, -1.0)),
        "max_force NaN": drives((1, capi.DRIVE_VELOCITY, 0.5, 0.0, nan)),
    }


def bad_slider_limit_cases():
    return {
        "slide limit on a hinge": limits((0, capi.LIMIT_SLIDE, -0.1, 0.1)),
        "two slide limits": limits((1, capi.LIMIT_SLIDE, -0.1, 0.1), (1, capi.LIMIT_SLIDE, -0.2, 0.2)),
        "slide lower > upper": limits((1, capi.LIMIT_SLIDE, 0.1, -0.1)),
        "slide bound infinite": limits((1, capi.LIMIT_SLIDE, -0.1, INF)),
        "slide bound NaN": limits((1, capi.LIMIT_SLIDE, float("nan"), 0.1)),
    }


def test_bad_drives_are_rejected_and_the_previous_ones_stay():
    bodies, sid, joints, good = mechanism()
    free = run_world(capi.SCENE_BOXES, bodies, sid, joints, None, None, 10, 20)
    want = run_world(capi.SCENE_BOXES, bodies, sid, joints, None, good, 10, 20)
    assert not bits_equal(want, free)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        w.set_joints(joints)
        w.set_joint_drives(good)
        for name, bad in bad_drive_cases().items():
            with pytest.raises(capi.XpbdError) as e:
                w.set_joint_drives(bad)
            assert e.value.code == capi.E_INVALID, name
        for name, bad in bad_slider_limit_cases().items():
            with pytest.raises(capi.XpbdError) as e:
                w.set_joint_limits(bad)
            assert e.value.code == capi.E_INVALID, name
        w.set_joint_limits(limits((1, capi.LIMIT_SLIDE, -50.0, 50.0), (1, capi.LIMIT_HINGE, -math.pi, math.pi, Y, Y)))   # beyond pi in metres is fine
        for _ in range(10):
            w.step(DT, 20)
        assert bits_equal(w.download(), want)                           # `good` still acted (and those limits never bound)
        bad_joints = joints.copy()
        bad_joints["distance"][1] = 0.5                                 # a slider needs distance 0 ...
        with pytest.raises(capi.XpbdError) as e:
            w.set_joints(bad_joints)
        assert e.value.code == capi.E_INVALID
        bad_joints = joints.copy()
        bad_joints["axis_b"][1] = [2.0, 0.0, 0.0]                       # ... and unit axes
        with pytest.raises(capi.XpbdError) as e:
            w.set_joints(bad_joints)
        assert e.value.code == capi.E_INVALID
    with capi.World(mode=capi.MODE_FUSED) as w:                         # only XPBD_MODE_CONTACTS takes drives
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        with pytest.raises(capi.XpbdError) as e:
            w.set_joint_drives(good)
        assert e.value.code == capi.E_INVALID


def test_multi_world_rejects_bad_drives_before_any_collective():
    bodies, sid, joints, good = mechanism()
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=0.75) as mw:
        mw.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        with pytest.raises(capi.XpbdError) as e:
            mw.set_joint_drives(good)                                   # no joints uploaded yet
        assert e.value.code == capi.E_INVALID
        mw.upload(bodies, sid, 0, len(bodies), joints)
        mw.set_joint_drives(good)
        for name, bad in bad_drive_cases().items():
            with pytest.raises(capi.XpbdError) as e:
                mw.set_joint_drives(bad)
            assert e.value.code == capi.E_INVALID, name
        for _ in range(10):
            mw.step(DT, 20)
        got = mw.download()
        mw.upload(bodies, sid, 0, len(bodies), joints)                  # upload clears the drives
        for _ in range(10):
            mw.step(DT, 20)
        cleared = mw.download()
    assert bits_equal(got, run_world(capi.SCENE_BOXES, bodies, sid, joints, None, good, 10, 20))
    assert bits_equal(cleared, run_world(capi.SCENE_BOXES, bodies, sid, joints, None, None, 10, 20))
