"""The damping model (tests/damping_model.py) and its yardstick, without a device.

1. The yardstick.  The GPU tests expect what the committed oracle gives when it is run one substep at a time (a frame of dt = h
   with one substep) with the model's stage 7 applied after every call.  That is only a yardstick if the oracle per substep
   equals the oracle per frame bit for bit (the broadphase of a one-substep frame sees less travel; it must still find every pair
   that touches).  Shown first, on every scene used so; the restitution model (scene "pile_bouncing") likewise.
2. With all defaults the model is the oracle, bit for bit.
3. Drag against its closed form, bit for bit, and against exp(-c S h) within the derived bound.
4. Known answers of the joint dampers and the caps.
5. The drag coefficient of the sleeping test ("Damping"), determined here."""
import math

import numpy as np
import pytest

import damping_common as dc
import damping_model as dm
import oracle_binding as ob
import restitution_model as rm
import sleep_common as sc

POLYS = dc.polys()


# ---- 1. the yardstick -------------------------------------------------------------------------------------------------------
def plain_scenes():
    for name in ("pile", "chain", "chain_on_pile"):
        bodies, sid, joints = dc.scene(name)[:3]
        yield name, bodies, sid, joints, dc.SUBSTEPS, dc.FRAMES, 0
    bodies, sid, joints = dc.scene("chain_on_pile")[:3]
    yield "chain_on_pile_gjk", bodies, sid, joints, dc.SUBSTEPS, dc.FRAMES, 1
    bodies, sid = dc.squeeze_scene()
    yield "squeeze", bodies, sid, dc.NO_JOINTS, dc.SUBSTEPS, dc.SQUEEZE_FRAMES, 0
    bodies, sid = sc.stack_scene()
    yield "stack", bodies, sid, dc.NO_JOINTS, dc.SLEEP_SUBSTEPS, 3, 0


@pytest.mark.parametrize("name,bodies,sid,joints,substeps,frames,narrowphase", list(plain_scenes()), ids=[s[0] for s in plain_scenes()])
def test_oracle_per_substep_equals_oracle_per_frame(name, bodies, sid, joints, substeps, frames, narrowphase):
    per_frame = per_substep = bodies
    for f in range(frames):
        per_frame = ob.contacts_step_joints(per_frame, sid, POLYS, joints, dc.DT, substeps, dc.PAD, narrowphase=narrowphase)
        per_substep = dm.oracle_substeps(per_substep, sid, POLYS, joints, dc.DT, substeps, dc.PAD, narrowphase=narrowphase, on=False)
        assert per_frame.tobytes() == per_substep.tobytes(), (name, f)
    assert not np.isnan(per_frame).any()


def test_restitution_model_per_substep_equals_per_frame():
    bodies, sid = dc.pile_scene()
    e = [dc.RESTITUTION] * len(bodies)
    per_frame, per_substep = (rm.Model(bodies, sid, POLYS, e=e, ground_e=dc.RESTITUTION) for _ in range(2))
    for f in range(2):
        per_frame.step(dc.DT, dc.SUBSTEPS)
        for _ in range(dc.SUBSTEPS):
            per_substep.step(dc.H, 1)
        assert per_frame.bodies.tobytes() == per_substep.bodies.tobytes(), f
    assert per_frame.pair_entries + per_frame.ground_entries > 0         # something bounced


# ---- 2. all defaults: the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pile", "chain_on_pile"])
def test_the_model_with_all_defaults_is_the_oracle(name):
    bodies, sid, joints = dc.scene(name)[:3]
    n = len(bodies)
    zero_dampers = dm.dampers(*[(j, 0.0, 0.0) for j in range(len(joints))])
    want = got = bodies
    for f in range(2):
        want = ob.contacts_step_joints(want, sid, POLYS, joints, dc.DT, dc.SUBSTEPS, dc.PAD)
        got = dm.oracle_substeps(got, sid, POLYS, joints, dc.DT, dc.SUBSTEPS, dc.PAD, dm.rows(n), zero_dampers)
        assert got.tobytes() == want.tobytes(), f


def test_the_scenes_do_what_they_are_for():
    """Caps fire for some bodies and substeps and not for others; dampers make entries with counts 1 and 2; the damped frames
    differ from the undamped ones; nothing is NaN."""
    for name in dc.SCENES:
        damped, plain = dc.expected(name), dc.expected(name, damped=False)
        assert not np.isnan(damped[-1]).any(), name
        assert damped[0].tobytes() != plain[0].tobytes(), name
        fixed = [i for i in range(len(plain[0])) if dm.is_fixed(plain[0][i])]
        assert fixed and all(damped[-1][i].tobytes() == dc.scene(name)[0][i].tobytes() for i in fixed), name
    rows = dc.pile_rows()
    lin, _ = dc.speeds(dc.expected("pile", damped=False)[0])
    capped = np.isfinite(rows["max_linear_speed"])
    assert (lin[capped] > 1.5).any() and (lin[capped] < 1.5).any()         # the cap binds for some of the capped lanes only
    lin, _ = dc.speeds(dc.expected("pile")[0])
    assert lin[capped].max() <= 1.5 * (1.0 + 1e-15) and lin[~capped].max() > 1.5


# ---- 3. drag ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, 2.0, 5.0])
def test_drag_equals_its_closed_form_bit_for_bit_and_the_exponential_within_the_derived_bound(c):
    """A body alone in space, no forces: stage 7 is all that changes its velocities.

    Closed form: after S substeps v = v0 multiplied S times by s = 1.0 / (1.0 + h c), the very operations of the header.

    Against the exponential.  With x = h c > 0:  s^S = exp(-S ln(1 + x)) = exp(-S x) exp(y),  y = S (x - ln(1 + x)), and
    x - ln(1 + x) = x^2/2 - x^3/3 + x^4/4 - ... <= x^2/2 - x^3/3 + x^4/4 (alternating, decreasing for x < 1).  For 0 <= y <= 1,
    exp(y) - 1 <= y + y^2.  So the relative excess of s^S over exp(-c S h) is at most
    S x^2/2 - S x^3/3 + S x^4/4 + S^2 x^4/4  <=  S x^2/2   whenever  x/4 + S x/4 <= 1/3, i.e. (S + 1) h c <= 4/3,
    and it is never negative.  Rounding adds at most S + 2 roundings of 2^-53 each, far below the bound asserted."""
    substeps, frames = dc.SUBSTEPS, 4
    S, h = substeps * frames, dc.H
    assert (S + 1) * h * c <= 4.0 / 3.0
    bodies, sid = dc.kc.boxes(1, [[0.0, 0.0, 50.0]])
    bodies[0, 10:22] = 0.0                                            # no gravity
    bodies[0, 22:28] = [0.3, -1.1, 0.7, 0.2, 2.0, -0.9]
    rows = dm.rows(1, linear=c, angular=c)
    s = 1.0 / (1.0 + h * c)
    want = [float(x) for x in bodies[0, 22:28]]
    for _ in range(S):
        want = [x * s for x in want]
    # stage 7 alone, S times: the closed form to the bit, both velocities
    b = bodies
    for _ in range(S):
        b = dm.stage7(b, dc.NO_JOINTS, h, rows)
    assert b[0, 22:28].tobytes() == np.array(want).tobytes()
    assert b[0, 0:22].tobytes() == bodies[0, 0:22].tobytes() and b[0, 28:38].tobytes() == bodies[0, 28:38].tobytes()
    for k in range(6):
        exact = float(bodies[0, 22 + k]) * math.exp(-c * S * h)
        excess = b[0, 22 + k] / exact - 1.0
        assert -1e-14 <= excess <= S * (h * c) ** 2 / 2.0, (k, excess)
    # behind the oracle's substeps: derive recomputes the velocity from the positions before and after (|x| < 64 m), two roundings
    # of ulp(64) / 2 each over h per substep; the angular velocity likewise from the rotation the body made, to first order
    b = bodies
    for _ in range(frames):
        b = dm.oracle_substeps(b, sid, POLYS, dc.NO_JOINTS, dc.DT, substeps, dc.PAD, rows)
    assert np.abs(b[0, 22:25] - want[0:3]).max() <= S * math.ulp(64.0) / h
    ratio = np.linalg.norm(b[0, 25:28]) / np.linalg.norm(bodies[0, 25:28])
    assert abs(ratio / s ** S - 1.0) < 1e-3


def test_zero_drag_and_infinite_caps_leave_every_bit():
    v = (1.0e-310, -0.0, 3.0e300)
    assert np.array(dm.drag_and_cap(v, dc.H, 0.0, dm.INF)).tobytes() == np.array(v).tobytes()


# ---- 4. known answers -------------------------------------------------------------------------------------------------------
def _pair(w_a, w_b, fixed_a=True):
    bodies, sid = dc.kc.boxes(2, [[0.0, 0.0, 5.0], [1.2, 0.0, 5.0]], fixed=[0] if fixed_a else [])
    bodies[0, 25:28], bodies[1, 25:28] = w_a, w_b
    joints = np.zeros(1, dtype=dc.capi.JOINT_DTYPE)
    joints[0]["body_a"], joints[0]["body_b"] = 0, 1
    joints[0]["anchor_a"], joints[0]["anchor_b"] = [1.1, 0.5, 0.5], [-0.1, 0.5, 0.5]
    return bodies, joints


def test_an_angular_damper_with_mu_h_of_one_or_more_stops_the_relative_spin_of_an_isotropic_box():
    bodies, joints = _pair([0.0, 0.0, 0.0], [0.4, -2.0, 1.0])
    out = dm.stage7(bodies, joints, dc.H, joint_damping=dm.dampers((0, 0.0, 1.0 / dc.H)))
    assert np.abs(out[1, 25:28]).max() <= 1e-15 * 3.0 and out[0].tobytes() == bodies[0].tobytes()
    half = dm.stage7(bodies, joints, dc.H, joint_damping=dm.dampers((0, 0.0, 0.5 / dc.H)))
    assert np.allclose(half[1, 25:28], 0.5 * bodies[1, 25:28], rtol=1e-14, atol=0.0)


def test_two_free_ends_meet_in_the_middle_and_keep_their_momentum():
    bodies, joints = _pair([1.0, 0.0, 0.0], [-1.0, 0.5, 0.0], fixed_a=False)
    out = dm.stage7(bodies, joints, dc.H, joint_damping=dm.dampers((0, 0.0, 2.0 / dc.H)))
    assert np.allclose(out[0, 25:28], out[1, 25:28], atol=1e-15)
    assert np.allclose(out[0, 25:28] + out[1, 25:28], bodies[0, 25:28] + bodies[1, 25:28], atol=1e-15)
    bodies[0, 22:25], bodies[1, 22:25] = [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]
    lin = dm.stage7(bodies, joints, dc.H, joint_damping=dm.dampers((0, 1.0 / dc.H, 0.0)))
    mass = 1.0 / bodies[0, 0]
    assert np.allclose(mass * (lin[0, 22:25] + lin[1, 22:25]), 0.0, atol=1e-12)          # opposite impulses of one size


def test_a_cap_leaves_the_direction_and_the_length_of_the_cap():
    v = dm.drag_and_cap((3.0, -4.0, 12.0), dc.H, 0.0, 6.5)
    assert math.sqrt(sum(x * x for x in v)) <= 6.5 * (1.0 + 1e-15) and np.allclose(v, [1.5, -2.0, 6.0], rtol=1e-15)
    assert dm.drag_and_cap((3.0, -4.0, 12.0), dc.H, 0.0, 13.0) == (3.0, -4.0, 12.0)       # m > cap is false at m == cap


# ---- 5. the drag that lets the 3-stack sleep --------------------------------------------------------------------------------
def stack_frame_under(c, budget):
    """The first frame (1-based) from which on every box of the 3-stack stays under half of both thresholds until frame `budget`,
    by the model with drag c on every body; None if the last frame is not under them."""
    bodies, sid = sc.stack_scene()
    rows = dm.rows(len(bodies), linear=c, angular=c)
    b, since = bodies, None
    for f in range(1, budget + 1):
        b = dm.oracle_substeps(b, sid, POLYS, dc.NO_JOINTS, dc.DT, dc.SLEEP_SUBSTEPS, dc.PAD, rows)
        lin, ang = dc.speeds(b[list(sc.STACK)])
        under = lin.max() < 0.5 * dc.SLEEP_CFG[0] and ang.max() < 0.5 * dc.SLEEP_CFG[1]
        since = (since or f) if under else None
    return since


def test_the_sleeping_tests_drag_is_the_smallest_candidate_that_calms_the_stack():
    found = None
    for c in dc.SLEEP_CANDIDATES:
        frame = stack_frame_under(c, dc.SLEEP_MODEL_BUDGET)
        print("drag %g 1/s: under half the thresholds after frame %s" % (c, frame))
        if frame is not None:
            found = (c, frame)
            break
    assert found == (dc.SLEEP_DRAG, dc.SLEEP_MODEL_FRAME), found
