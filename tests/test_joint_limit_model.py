"""The joint-limit model (tests/joint_limit_model.py) on CPU: its joint pass agrees with the oracle where the oracle
defines one (no limits), its angles are the ones include/xpbd.h names, and a limited hinge stops a spinning door."""
import math

import numpy as np
import pytest

import joint_limit_model as jm
import oracle_binding as ob
from constraint_solver_amd import capi

DT = 1.0 / 60.0
POLYS = ob.polytopes_array([("cube", 1.0)])
Z = [0.0, 0.0, 1.0]


def quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[math.cos(angle / 2)], axis * math.sin(angle / 2)])


def random_scene(seed, n_bodies=6):
    """A row of free cubes 1.6 m apart (no contact), tilted and spinning, no gravity, linked by ball / distance / hinge
    joints between neighbours: every body touches nothing for a frame."""
    rng = np.random.default_rng(seed)
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, n_bodies)
    bodies[:, 10:22] = 0.0
    for i in range(n_bodies):
        bodies[i, 31:34] = [1.6 * i, 0.0, 3.0]
        bodies[i, 34:38] = quat(rng.normal(size=3), rng.uniform(-0.2, 0.2))
        bodies[i, 22:25] = rng.normal(scale=0.3, size=3)
        bodies[i, 25:28] = rng.normal(scale=1.0, size=3)
    bodies[0, 0:10] = 0.0                                        # one static body
    joints = np.zeros(n_bodies - 1, dtype=capi.JOINT_DTYPE)
    for k in range(n_bodies - 1):
        j = joints[k]
        j["body_a"], j["body_b"] = k, k + 1
        j["anchor_a"], j["anchor_b"] = [1.3, 0.5, 0.5], [-0.3, 0.5, 0.5]
        j["distance"] = 0.0 if k % 3 else 0.05
        if k % 2:
            axis = rng.normal(size=3)
            j["axis_a"] = j["axis_b"] = axis / np.linalg.norm(axis)
            j["kind"] = capi.JOINT_HINGE
    return bodies, sid, joints


@pytest.mark.parametrize("seed", range(4))
def test_model_without_limits_matches_the_oracle(seed):
    bodies, sid, joints = random_scene(seed)
    want = ob.contacts_step_joints(bodies, sid, POLYS, joints, DT, 20, 0.02)
    got = jm.step(bodies, joints, np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE), DT, 20)
    assert np.abs(want - bodies).max() > 1e-3                    # the joints did something
    np.testing.assert_allclose(got[:, 31:38], want[:, 31:38], rtol=0, atol=1e-12)
    # velocities are pose differences over h = 1/1200 s: a pose rounding of 1e-15 shows there as 1e-12
    np.testing.assert_allclose(got[:, 22:28], want[:, 22:28], rtol=0, atol=1e-11)
    assert np.array_equal(got[:, :22], bodies[:, :22]) and np.array_equal(got[:, 28:31], bodies[:, 28:31])


def angle(kind, q_a, q_b, axis_a=Z, axis_b=Z, ref_a=(1.0, 0.0, 0.0), ref_b=(1.0, 0.0, 0.0)):
    return jm.limit_angle(kind, np.asarray(q_a), np.asarray(q_b), axis_a, axis_b, ref_a, ref_b)


IDENTITY = [1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("theta", [0.7, -0.7, 3.1, -3.1, math.pi - 1e-9, -(math.pi - 1e-9)])
def test_hinge_angle_is_the_signed_turn_of_b_about_the_axis(theta):
    phi, n = angle(jm.LIMIT_HINGE, IDENTITY, quat(Z, theta))
    assert phi == pytest.approx(theta, abs=1e-12)
    np.testing.assert_allclose(n, Z, atol=1e-15)
    phi, _ = angle(jm.LIMIT_HINGE, quat(Z, theta), IDENTITY)     # a turned instead: the opposite sign
    assert phi == pytest.approx(-theta, abs=1e-12)


def test_hinge_angle_wraps_past_pi():
    phi, _ = angle(jm.LIMIT_HINGE, IDENTITY, quat(Z, math.pi + 0.1))
    assert phi == pytest.approx(-(math.pi - 0.1), abs=1e-12)


@pytest.mark.parametrize("theta", [0.5, -0.5, 3.1, -3.1])
def test_swing_angle_is_the_angle_between_the_axes(theta):
    phi, n = angle(jm.LIMIT_SWING, IDENTITY, quat([1.0, 0.0, 0.0], theta))
    assert phi == pytest.approx(abs(theta), abs=1e-12)
    np.testing.assert_allclose(n, [math.copysign(1.0, theta), 0.0, 0.0], atol=1e-12)
    assert angle(jm.LIMIT_SWING, quat(Z, 0.3), quat(Z, -1.0)) is None   # aligned axes: no entry


@pytest.mark.parametrize("theta", [0.4, -0.4, 3.1, -3.1])
def test_twist_angle_is_the_turn_about_the_bisector(theta):
    phi, n = angle(jm.LIMIT_TWIST, quat(Z, -theta / 2), quat(Z, theta / 2))
    assert phi == pytest.approx(theta, abs=1e-12)
    np.testing.assert_allclose(n, Z, atol=1e-15)


@pytest.mark.parametrize("swing_axis", [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
def test_a_pure_swing_is_no_twist(swing_axis):
    phi, _ = angle(jm.LIMIT_TWIST, IDENTITY, quat(swing_axis, 0.9))
    assert phi == pytest.approx(0.0, abs=1e-12)
    phi, _ = angle(jm.LIMIT_TWIST, quat(Z, -0.2), quat(Z, 0.2))   # ... and a pure twist is no swing
    assert angle(jm.LIMIT_SWING, quat(Z, -0.2), quat(Z, 0.2)) is None and phi == pytest.approx(0.4, abs=1e-12)


def test_opposite_axes_define_no_twist():
    assert angle(jm.LIMIT_TWIST, IDENTITY, [0.0, 1.0, 0.0, 0.0]) is None   # b turned by exactly pi about x


def door_scene(spin):
    """A cube door on a static post, hinged on the vertical line x = 1.3, y = 0 (tests/test_joints_oracle.py)."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 2)
    bodies[:, 34:38] = IDENTITY
    bodies[:, 10:28] = 0.0
    bodies[0, 0:10] = 0.0
    bodies[0, 31:34] = [0.0, 0.0, 5.0]
    bodies[1, 31:34] = [1.6, 0.0, 5.0]
    bodies[1, 27] = spin
    joints = np.zeros(1, dtype=capi.JOINT_DTYPE)
    joints["body_b"] = 1
    joints["anchor_a"], joints["anchor_b"] = [1.3, 0.0, 0.5], [-0.3, 0.0, 0.5]
    joints["axis_a"] = joints["axis_b"] = Z
    joints["kind"] = capi.JOINT_HINGE
    return bodies, sid, joints


def hinge_limit(lower, upper):
    lim = np.zeros(1, dtype=capi.JOINT_LIMIT_DTYPE)
    lim["kind"] = capi.LIMIT_HINGE
    lim["ref_a"] = lim["ref_b"] = [1.0, 0.0, 0.0]
    lim["lower"], lim["upper"] = lower, upper
    return lim


def door_angle(bodies):
    return angle(jm.LIMIT_HINGE, bodies[0, 34:38], bodies[1, 34:38])[0]


@pytest.mark.parametrize("spin,stop", [(20.0, 0.6), (-20.0, -0.4)])
def test_model_door_spun_into_a_hinge_stop_stops_there(spin, stop):
    """The door reaches the stop it is spun towards and never passes it by more than 0.02 rad.  (It does not stay there:
    the Jacobi average of its positional and limit terms gives the stop some give, and the door comes back off it.)"""
    bodies, _, joints = door_scene(spin)
    lim = hinge_limit(-0.4, 0.6)
    b, seen = bodies, []
    for _ in range(60):
        b = jm.step(b, joints, lim, DT, 20)
        seen.append(door_angle(b))
    assert -0.42 <= min(seen) and max(seen) <= 0.62
    assert min(abs(phi - stop) for phi in seen) < 0.02
    free = bodies
    for _ in range(20):
        free = jm.step(free, joints, np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE), DT, 20)
    assert abs(door_angle(free)) > 1.0                            # without the stop it turns on
