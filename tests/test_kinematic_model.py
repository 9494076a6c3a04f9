"""The kinematic model (tests/kinematic_model.py) and its yardstick, without a device.

1. The yardstick.  The GPU tests expect what the committed oracle gives when it is run one substep at a time (a frame of
   dt = h with one substep) with the model's velocities written into the kinematic bodies before every call.  That is only a
   yardstick if, with the platform held static, the oracle per substep equals the oracle per frame bit for bit (the broadphase
   of a one-substep frame sees less travel; it must still find every pair that touches).  Shown first, on every scene used so.
2. Known answers of the model: a POSE target is reached after S substeps for S in {1, 3, 20}.
3. Position arrival against exact rational arithmetic, with the bound derived below.
4. What the set_dynamics substitute loses: a fixed body given an angular velocity keeps (2 / h) sin(atan(h |w| / 2)) of it per
   substep, the model's VELOCITY mode keeps all of it."""
import math
from fractions import Fraction

import numpy as np
import pytest

import kinematic_common as kc
import kinematic_model as km
import oracle_binding as ob

POLYS = ob.polytopes_array(kc.POLY_NAMES)


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------
def static_scenes():
    yield "carry", kc.carry_scene(), kc.CARRY_SUBSTEPS, 3
    yield "velocity", kc.velocity_scene()[:2], kc.VELOCITY_SUBSTEPS, 3
    yield "stacks", kc.stacks_scene(), kc.SLEEP_SUBSTEPS, 2
    bodies, sid, _ = kc.retarget_scene()
    keep = [0, 3, kc.N_PLATFORMS, kc.N_PLATFORMS + 1]               # two platforms with their riders: the rest repeat them
    yield "retarget", (bodies[keep], sid[keep]), kc.RETARGET_SUBSTEPS, 3


@pytest.mark.parametrize("name,scene,substeps,frames", list(static_scenes()), ids=[s[0] for s in static_scenes()])
def test_oracle_per_substep_equals_oracle_per_frame_with_the_platform_static(name, scene, substeps, frames):
    bodies, sid = scene
    per_frame = per_substep = bodies
    for f in range(frames):
        per_frame = ob.contacts_step_joints(per_frame, sid, POLYS, kc.NO_JOINTS, kc.DT, substeps, kc.PAD)
        per_substep = km.oracle_substeps(per_substep, sid, POLYS, kc.NO_JOINTS, kc.DT, substeps, kc.PAD)
        assert per_frame.tobytes() == per_substep.tobytes(), (name, f)
    moved = np.abs(per_frame[:, 31:34] - bodies[:, 31:34]).max(axis=1)
    assert (moved > 0.0).any() and not np.isnan(per_frame).any()      # somebody settled: the scene has contacts at work


def test_a_held_pose_entry_is_a_static_platform_bit_for_bit():
    """POSE with target == pose gives zero velocities: the model's frames are the plain oracle's."""
    bodies, sid = kc.carry_scene()
    want = got = bodies
    for tbl in kc.carry_tables(static=True)[:3]:
        want = ob.contacts_step_joints(want, sid, POLYS, kc.NO_JOINTS, kc.DT, kc.CARRY_SUBSTEPS, kc.PAD)
        got = km.oracle_substeps(got, sid, POLYS, kc.NO_JOINTS, kc.DT, kc.CARRY_SUBSTEPS, kc.PAD, tbl)
        assert got.tobytes() == want.tobytes()


def test_the_carried_box_keeps_more_than_half_the_slabs_displacement():
    frames = kc.carry_expected()
    slab = frames[-1][0, 31] - 0.0
    box = frames[-1][1, 31] - 0.0
    assert slab == kc.CARRY_STEP * kc.CARRY_FRAMES                    # the slab arrives on the bit: translation only
    assert box > 0.5 * slab, (box, slab)
    assert abs(frames[-1][1, 33] - (kc.SLAB_Z + 1.0)) < 0.2 and not np.isnan(frames[-1]).any()      # and is still on it


# ---- 2. known answers ---------------------------------------------------------------------------------------------------
def ulp_bound(p, p_t):
    return 4.0 * math.ulp(max(abs(p), abs(p_t)))


# Rotation arrival.  The last substep (r = 1) aims at q_t from wherever the earlier ones left the body, so only its own errors
# remain: the product q_t * conj(q) and its length (4 roundings each component, relative 2^-53 each), atan2 and tan (an ulp each
# on a libm that is not correctly rounded), the division and products of the scale (4), and the rotation update with its
# normalisation (about 8 per component).  tan is evaluated at half <= pi / 2, where the update undoes it through
# normalized(q + tan(half) n q): an error d in tan moves the angle by d / (1 + tan^2), never more than d relative.  Some 24
# roundings of 2^-53 on components of size <= 1: 32 ulp of 1.0 (2^-52 each) leaves a factor of two.
ROTATION_BOUND = 32 * 2.0 ** -52


@pytest.mark.parametrize("substeps", kc.ARRIVAL_SUBSTEPS)
def test_a_pose_target_is_reached_after_s_substeps(substeps):
    bodies, _, tbl = kc.arrival_scene()
    got = kc.arrival_model(substeps)
    worst = 0.0
    for i in range(kc.N_ARRIVAL):
        p_t, q_t = tbl[i]["linear"], tbl[i]["angular"]
        for c in range(3):
            assert abs(got[i, c] - p_t[c]) <= ulp_bound(bodies[i, 31 + c], p_t[c]), (i, c)
        unit = q_t / math.sqrt(float(np.dot(q_t, q_t)))
        q = got[i, 3:7]
        dev = min(np.abs(q - unit).max(), np.abs(q + unit).max())   # q and -q are one rotation
        worst = max(worst, float(dev))
    print("substeps %d: largest rotation miss %.3g (bound %.3g)" % (substeps, worst, ROTATION_BOUND))
    assert worst <= ROTATION_BOUND


@pytest.mark.parametrize("substeps", kc.ARRIVAL_SUBSTEPS)
def test_the_special_entries_are_what_they_claim(substeps):
    bodies, _, tbl = kc.arrival_scene()
    q, q_t = bodies[kc.HALF_TURN, 34:38], tbl[kc.HALF_TURN]["angular"]
    assert km.qmul(tuple(q_t), (q[0], -q[1], -q[2], -q[3]))[0] == 0.0                         # dq.s == 0
    assert abs(float(np.linalg.norm(tbl[kc.UNNORMALISED]["angular"])) - 3.7) < 1e-12
    assert np.array_equal(tbl[kc.MINUS_Q]["angular"], -bodies[kc.MINUS_Q, 34:38])
    h = kc.DT / substeps
    _, ang = km.pose_velocities(tuple(bodies[kc.MINUS_Q, 31:34]), tuple(bodies[kc.MINUS_Q, 34:38]), tuple(tbl[kc.MINUS_Q]["linear"]),
                                tuple(tbl[kc.MINUS_Q]["angular"]), h, substeps)
    assert max(abs(x) for x in ang) * h < 1e-14                       # the same rotation: (next to) no turn


# ---- 3. position arrival against exact arithmetic -----------------------------------------------------------------------
def test_position_arrival_is_within_four_ulp_of_exact():
    """In the last substep  p' = p + h * ((p_t - p) / (1.0 * h)).  1.0 * h is exact, so four operations round: the difference d,
    the quotient, the product, the sum.  The first three each add at most 2^-53 |d| relative to the exact d (which the exact
    arithmetic below returns to p_t - p exactly), the sum half an ulp of the result: for p and p_t of one sign |d| <= max(|p|,
    |p_t|) and the total stays below 3.5 ulp of that maximum; the bound asserted is 4.  Checked against Fractions for 20 000
    random (p, p_t, h), both signs, magnitudes from 1e-3 to 1e6, and r = 1..20 substeps run in sequence."""
    rng = np.random.default_rng(4000)
    worst = 0.0
    for _ in range(20000):
        scale = 10.0 ** rng.uniform(-3.0, 6.0)
        p0, p_t = float(rng.uniform(-scale, scale)), float(rng.uniform(-scale, scale))
        substeps = int(rng.integers(1, 21))
        h = float(rng.uniform(1e-4, 1e-1)) / substeps
        p = p0
        for k in range(substeps):
            vel = (p_t - p) / (float(substeps - k) * h)
            p = p + h * vel
        err = abs(Fraction(p) - Fraction(p_t))
        ulp = Fraction(math.ulp(max(abs(p0), abs(p_t))))
        worst = max(worst, float(err / ulp))
        assert err <= 4 * ulp, (p0, p_t, h, substeps, float(err / ulp))
    print("largest miss %.3f ulp of max(|p|, |p_t|)" % worst)


# ---- 4. the substitute decays, VELOCITY mode does not -------------------------------------------------------------------
def test_a_fixed_body_given_an_angular_velocity_decays_and_velocity_mode_does_not():
    h, w0 = kc.DT / 20, (0.0, 3.0, -1.0)
    speed0 = math.sqrt(sum(x * x for x in w0))
    q, w = kc.IDENT, w0
    for _ in range(20):                                               # no overwrite: what set_dynamics on a fixed body gives
        past = q
        _, q = km.integrate_pose((0.0, 0.0, 0.0), q, (0.0, 0.0, 0.0), w, h)
        w = km.derive_angular(q, past, h)
        speed = math.sqrt(sum(x * x for x in w))
    per_substep = (2.0 / h) * math.sin(math.atan(h * speed0 / 2.0)) / speed0
    assert speed < speed0 and abs(speed / speed0 - per_substep ** 20) < 1e-3 * (1.0 - per_substep ** 20)   # (the factor itself creeps up as the speed falls)
    entry = km.table((0, km.VELOCITY, [0.0, 0.0, 0.0], w0))[0]
    after = km.fly((0.0, 0.0, 0.0), kc.IDENT, entry, kc.DT, 20)
    turned = 2.0 * math.atan2(math.sqrt(sum(x * x for x in after[0][1][1:])), after[0][1][0])
    assert abs(turned - 2.0 * math.atan(h * speed0 / 2.0)) < 1e-15    # a substep turns the body by 2 atan(h |w| / 2), not h |w|
    left = [math.sqrt(sum(x * x for x in step[3])) for step in after]
    assert max(left) - min(left) < 1e-12 * speed0                    # every substep leaves the same speed behind: no decay
