"""The independent model of xpbd_world_joint_states (tests/joint_state_model.py) on known answers, and the scenes of the GPU
tests (tests/joint_state_common.py) checked on the CPU: stepped by the joint model, every bound of every limit stays at least
1e-6 away from the angle or travel it is compared with, so the limit bits the device reports cannot hinge on rounding; and
between them the scenes show every joint, limit and drive kind and every flag."""
import math

import numpy as np
import pytest

import joint_drive_model as jd
import joint_state_common as jc
import joint_state_model as jsm

X, Y, Z = jd.X, jd.Y, jd.Z
PI = math.pi


def about(axis, angle):
    return np.concatenate([[math.cos(angle / 2)], np.asarray(axis, dtype=np.float64) * math.sin(angle / 2)])


def qmul(p, q):
    return np.concatenate([[p[0] * q[0] - np.dot(p[1:], q[1:])], p[0] * q[1:] + q[0] * p[1:] + np.cross(p[1:], q[1:])])


def state(rows, joints, limits=jd.NO_LIMITS, drives=jd.NO_DRIVES):
    return jsm.joint_states(rows, joints, limits, drives)[0][0]


def encoder(axis):
    ref = jd.perpendicular_to(axis)
    return jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_HINGE, ref_a=ref, ref_b=ref, lower=-PI, upper=PI))


def test_a_hinge_turned_by_a_known_angle_reads_it():
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_HINGE, Z)
    rows[1, 34:38] = about(Z, 0.3)
    st = state(rows, joints, encoder(Z))
    assert abs(st["angle"] - 0.3) < 1e-15 and st["flags"] == jsm.HAS_ANGLE and st["kind"] == jd.JOINT_HINGE
    assert st["separation"] == 0.0 and abs(st["misalignment"]) < 1e-16 and st["travel"] == 0.0 and st["swing"] == 0.0
    bare = state(rows, joints)                                         # no references: no angle
    assert bare["flags"] == 0 and bare["angle"] == 0.0 and bare["angle_rate"] == 0.0
    tight = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_HINGE, ref_a=X, ref_b=X, lower=-0.1, upper=0.2))
    assert state(rows, joints, tight)["flags"] == jsm.HAS_ANGLE | jsm.ANGLE_ABOVE
    rows[1, 34:38] = about(Z, -0.3)
    assert state(rows, joints, tight)["flags"] == jsm.HAS_ANGLE | jsm.ANGLE_BELOW


def test_the_drives_references_win_and_the_limit_bits_keep_the_limits_own():
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_HINGE, Z)
    rows[1, 34:38] = about(Z, 0.3)
    limit = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_HINGE, ref_a=X, ref_b=X, lower=-0.1, upper=0.2))
    drive = jd.records(jd.DRIVE_DTYPE, dict(joint=0, kind=jd.DRIVE_ANGLE, ref_a=X, ref_b=Y, target=0.0, max_force=jd.INF))
    st = state(rows, joints, limit, drive)                             # from X on a to Y on b: a quarter turn further
    assert abs(st["angle"] - (0.3 + PI / 2)) < 1e-15
    assert st["flags"] == jsm.HAS_ANGLE | jsm.ANGLE_OF_DRIVE | jsm.ANGLE_ABOVE


def test_a_slider_moved_along_its_axis_reads_the_travel():
    axis = np.array([math.cos(0.5), 0.0, -math.sin(0.5)])
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_SLIDER, axis)
    rows[1, 31:34] += 0.25 * axis
    rows[1, 22:25] = 0.75 * axis + 2.0 * np.cross(axis, Y)             # only the part along the axis is travel_rate
    st = state(rows, joints)
    assert abs(st["travel"] - 0.25) < 1e-15 and abs(st["travel_rate"] - 0.75) < 1e-15 and abs(st["separation"]) < 1e-15
    assert st["flags"] == jsm.HAS_TRAVEL
    stop = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_SLIDE, lower=-0.3, upper=0.2))
    assert state(rows, joints, stop)["flags"] == jsm.HAS_TRAVEL | jsm.TRAVEL_ABOVE
    rows[1, 31:34] += 0.1 * np.cross(axis, Y)                          # off the axis: the perpendicular term's len
    assert abs(state(rows, joints)["separation"] - 0.1) < 1e-15


def test_a_wheel_spun_at_a_known_rate_reads_it():
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_HINGE, Z)
    rows[1, 25:28] = [0.4, -0.2, 3.0]
    assert abs(state(rows, joints, encoder(Z))["angle_rate"] - 3.0) < 1e-15
    rows[0, 25:28] = [0.0, 0.0, 1.0]                                   # relative to the base
    assert abs(state(rows, joints, encoder(Z))["angle_rate"] - 2.0) < 1e-15
    # ... and the driven wheel of the joint model turns at its drive's speed, as derive reports a speed: off the vector part of the
    # substep's rotation, 2 sin(theta / 2) / h, which is short of theta / h by theta^2 / 24 of it (theta = 3 rad/s * h, h = 1 / 1200:
    # 7.8e-7 rad/s; the bound leaves room for four times that)
    _, scene_joints, limits, drives, _, _, _ = jd.scene("wheel")
    st = state(jd.run_scene("wheel")[-1], scene_joints, limits, drives)
    assert st["flags"] == jsm.HAS_ANGLE | jsm.ANGLE_OF_DRIVE and abs(st["angle_rate"] - jd.WHEEL_SPEED) < 3.2e-6


def test_swing_and_twist_built_by_construction_read_back():
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_DISTANCE, Z)
    swing_only = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_SWING, lower=0.0, upper=0.3))
    twist_only = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_TWIST, ref_a=X, ref_b=X, lower=-0.5, upper=0.1))
    both = np.concatenate([twist_only, swing_only])
    rows[1, 34:38] = about(X, 0.4)                                     # pure swing
    st = state(rows, joints, swing_only)
    assert abs(st["swing"] - 0.4) < 1e-15 and st["flags"] == jsm.HAS_SWING | jsm.SWING_ABOVE and st["twist"] == 0.0
    rows[1, 34:38] = about(Z, 0.25)                                    # pure twist: the swing is reported beside it
    st = state(rows, joints, twist_only)
    assert abs(st["twist"] - 0.25) < 1e-15 and abs(st["swing"]) < 1e-15
    assert st["flags"] == jsm.HAS_SWING | jsm.HAS_TWIST | jsm.TWIST_ABOVE
    # a twist tau about b's own axis, then a swing theta about x: about the bisector the references are tan(phi) = tan(tau) cos(theta / 2) apart
    theta, tau = 0.4, -0.7
    rows[1, 34:38] = qmul(about(X, theta), about(Z, tau))
    st = state(rows, joints, both)
    assert abs(st["swing"] - theta) < 1e-15
    assert abs(st["twist"] - math.atan2(math.sin(tau) * math.cos(theta / 2), math.cos(tau))) < 1e-15
    assert st["flags"] == jsm.HAS_SWING | jsm.HAS_TWIST | jsm.SWING_ABOVE | jsm.TWIST_BELOW
    assert state(rows, joints)["flags"] == 0                           # a ball joint without limits reports neither
    rows[1, 34:38] = [1.0, 0.0, 0.0, 0.0]                              # exactly opposed axes: no bisector, no twist
    joints["axis_b"] = [0.0, 0.0, -1.0]
    st = state(rows, joints, both)
    assert st["flags"] == jsm.HAS_SWING and st["twist"] == 0.0 and st["swing"] == PI


def test_a_ball_joint_reports_its_positional_error():
    rows, joints = jd.two_rows(), jd.one_joint(jd.JOINT_DISTANCE, Z)
    joints["distance"] = 0.3
    rows[1, 31:34] += [0.0, 0.4, 0.3]
    st = state(rows, joints)
    assert abs(st["separation"] - 0.2) < 1e-15 and st["misalignment"] == 0.0 and st["flags"] == 0


# ---- the scenes of the GPU tests, stepped by the joint model ------------------------------------------------------------
ALL_FLAGS = (jsm.HAS_ANGLE | jsm.HAS_TRAVEL | jsm.HAS_SWING | jsm.HAS_TWIST | jsm.ANGLE_OF_DRIVE | jsm.ANGLE_BELOW | jsm.ANGLE_ABOVE |
             jsm.TRAVEL_BELOW | jsm.TRAVEL_ABOVE | jsm.SWING_ABOVE | jsm.TWIST_BELOW | jsm.TWIST_ABOVE)
_SEEN = {"flags": 0, "kinds": set()}


def model_states(n_joints, seed):
    bodies, _, joints, lims, drvs = jc.mechanisms(n_joints, seed)
    rows = bodies
    for _ in range(jc.FRAMES):
        rows = jd.step(rows, joints, lims, drvs, jc.DT, jc.SUBSTEPS)
    states, margin = jsm.joint_states(rows, joints, lims, drvs)
    _SEEN["flags"] |= int(np.bitwise_or.reduce(states["flags"]))
    _SEEN["kinds"] |= {("joint", int(k)) for k in joints["kind"]} | {("limit", int(k)) for k in lims["kind"]} | {("drive", int(k)) for k in drvs["kind"]}
    return states, margin


@pytest.mark.parametrize("n_joints,seeds", [(1, range(jc.N_RECIPES))] + [(n, [0]) for n in jc.STATE_WORLDS])
def test_no_bound_of_the_gpu_scenes_is_within_1e_6_of_its_angle(n_joints, seeds):
    for seed in seeds:
        states, margin = model_states(n_joints, seed)
        print("%d joints, seed %d: the nearest bound is %.3g away" % (n_joints, seed, margin))
        assert margin >= 1e-6, (n_joints, seed, margin)
        assert np.isfinite(np.array([states[name] for name in jsm.DOUBLES])).all()


def test_the_gpu_scenes_show_every_kind_and_every_flag():
    model_states(jc.STATE_WORLDS[0], 0)                                # (alone, this test still sees a whole world)
    assert _SEEN["flags"] == ALL_FLAGS, hex(_SEEN["flags"] ^ ALL_FLAGS)
    assert _SEEN["kinds"] == ({("joint", k) for k in range(3)} | {("limit", k) for k in range(4)} | {("drive", k) for k in range(4)})
