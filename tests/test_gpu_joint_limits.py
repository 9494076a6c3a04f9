"""Angular joint limits (xpbd_world_set_joint_limits, xpbd_multi_world_set_joint_limits) on the GPU: limits that never bind
change no bit, the stops hold, the device agrees with the independent model (tests/joint_limit_model.py), a sharded world
equals the single one bit for bit, and bad arguments are rejected with the previous limits left in place."""
import math

import numpy as np
import pytest

import joint_limit_model as jm
import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import chain_joints, expected, line_scene

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
X, Y, Z = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
NO_LIMITS = np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE)


def limits(*rows):
    """rows of (joint, kind, lower, upper[, ref_a, ref_b])"""
    out = np.zeros(len(rows), dtype=capi.JOINT_LIMIT_DTYPE)
    for k, r in enumerate(rows):
        out[k]["joint"], out[k]["kind"], out[k]["lower"], out[k]["upper"] = r[:4]
        out[k]["ref_a"], out[k]["ref_b"] = (r[4], r[5]) if len(r) > 4 else (X, X)
    return out


def pile(kind, n, seed, width, height):
    rng = np.random.default_rng(seed)
    bodies, sid = capi.scene_generate(kind, seed, n)
    bodies[:, 31:33] = rng.uniform(0, width, (n, 2))
    bodies[:, 33] = rng.uniform(0.5, height, n)
    bodies[:, 22:25] *= 0.3
    return bodies, sid


def run_world(kind, bodies, sid, joints, lims, frames, substeps):
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies, sid)
        w.set_joints(joints)
        if lims is not None:
            w.set_joint_limits(lims)
        for _ in range(frames):
            w.step(DT, substeps)
        return w.download()


# ---- 1. limits that never bind change nothing -------------------------------------------------------------------------
@pytest.mark.parametrize("n,width,frames", [(160, 4.0, 30), (SMALL_WORLD + 200, 140.0, 4)])
def test_never_binding_limits_change_no_bit(n, width, frames):
    """The scene of test_gpu_pairs.py::test_joints_with_contacts_match_oracle (chain joints through a pile, with contacts), one
    joint made an XPBD_JOINT_HINGE; every joint gets limits that cannot bind.  At or below SMALL_WORLD bodies the pair solve
    runs eight lanes per body, above it one."""
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = pile(kind, n, 6, width, 6.0)
    joints = chain_joints(capi, n)
    joints["axis_a"], joints["axis_b"] = Z, Z
    joints["kind"][1] = capi.JOINT_HINGE
    rows = []
    for k in range(len(joints)):
        if k == 1:
            rows.append((k, capi.LIMIT_HINGE, -math.pi, math.pi))
        else:
            rows += [(k, capi.LIMIT_SWING, 0.0, math.pi), (k, capi.LIMIT_TWIST, -math.pi, math.pi)]
    want = expected(ob, bodies, sid, kind, 10, frames, 0.02, joints)
    plain = run_world(kind, bodies, sid, joints, None, frames, 10)
    got = run_world(kind, bodies, sid, joints, limits(*rows), frames, 10)
    assert bits_equal(plain, want)
    assert bits_equal(got, want)


# ---- 2. the stops hold ------------------------------------------------------------------------------------------------
def two_bodies(spin, kind, axis, anchor_a, anchor_b):
    """A static post and a free cube linked by one joint 0.5 m in front of the cube's face: within the limits below the cube
    cannot reach the post (no contact; no gravity)."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 2)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 10:28] = 0.0
    bodies[0, 0:10] = 0.0
    bodies[0, 31:34] = [0.0, 0.0, 5.0]
    bodies[1, 31:34] = [2.5, 0.0, 5.0]
    bodies[1, 25:28] = spin
    joints = np.zeros(1, dtype=capi.JOINT_DTYPE)
    joints["body_b"], joints["kind"] = 1, kind
    joints["anchor_a"], joints["anchor_b"] = anchor_a, anchor_b
    joints["axis_a"] = joints["axis_b"] = axis
    return bodies, sid, joints


def trajectory(bodies, sid, joints, lims, frames=60):
    out = []
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        w.set_joints(joints)
        w.set_joint_limits(lims)
        for _ in range(frames):
            w.step(DT, 20)
            out.append(w.download())
    return out


def angle_of(b, joint, lim):
    got = jm.limit_angle(int(lim["kind"]), b[0, 34:38], b[1, 34:38], joint["axis_a"], joint["axis_b"], lim["ref_a"], lim["ref_b"])
    return 0.0 if got is None else got[0]


@pytest.mark.parametrize("spin,stop", [(20.0, 0.6), (-20.0, -0.4)])
def test_hinge_stop_holds_a_spinning_door(spin, stop):
    bodies, sid, joints = two_bodies([0.0, 0.0, spin], capi.JOINT_HINGE, Z, [2.0, 0.0, 0.5], [-0.5, 0.0, 0.5])
    lim = limits((0, capi.LIMIT_HINGE, -0.4, 0.6))
    seen = [angle_of(b, joints[0], lim[0]) for b in trajectory(bodies, sid, joints, lim)]
    assert -0.42 <= min(seen) and max(seen) <= 0.62
    assert min(abs(phi - stop) for phi in seen) < 0.02                 # it reached the stop it was spun towards
    free = [angle_of(b, joints[0], lim[0]) for b in trajectory(bodies, sid, joints, NO_LIMITS)]
    assert max(abs(phi) for phi in free) > 1.0                          # the control turns far past it


@pytest.mark.parametrize("spin", [[12.0, 0.0, 0.0], [0.0, 10.0, 0.0], [8.0, 6.0, -7.0], [-9.0, -5.0, 4.0]])
def test_swing_and_twist_limits_hold_a_spinning_ball_joint(spin):
    bodies, sid, joints = two_bodies(spin, capi.JOINT_DISTANCE, X, [2.0, 0.5, 0.5], [-0.5, 0.5, 0.5])
    lim = limits((0, capi.LIMIT_SWING, 0.0, 0.5, Y, Y), (0, capi.LIMIT_TWIST, -0.3, 0.3, Y, Y))

    def extremes(lims, frames=60):
        path = trajectory(bodies, sid, joints, lims, frames)
        return max(angle_of(b, joints[0], lim[0]) for b in path), max(abs(angle_of(b, joints[0], lim[1])) for b in path)

    swing, twist = extremes(lim)
    assert swing <= 0.52 and twist <= 0.32
    free_swing, free_twist = extremes(NO_LIMITS, 30)
    assert free_swing > 0.65 or free_twist > 0.6                        # the control goes far past them


# ---- 3. the device agrees with the model ------------------------------------------------------------------------------
def random_limited_scene(seed, n_bodies=6):
    """Free cubes in a row 2 m apart (their bounding spheres never meet), tilted and spinning, no gravity; hinge and ball
    joints between neighbours with tight limits that bind within the step."""
    rng = np.random.default_rng(1000 + seed)
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, n_bodies)
    bodies[:, 10:22] = 0.0
    rows = []
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
        if rng.uniform() < 0.5:
            j["kind"] = capi.JOINT_HINGE
            lo = rng.uniform(-0.2, 0.0)
            rows.append((k, capi.LIMIT_HINGE, lo, lo + rng.uniform(0.0, 0.2), ref, ref))
        else:
            choice = rng.integers(3)
            if choice != 1:
                rows.append((k, capi.LIMIT_SWING, 0.0, rng.uniform(0.0, 0.2)))
            if choice != 0:
                lo = rng.uniform(-0.2, 0.0)
                rows.append((k, capi.LIMIT_TWIST, lo, lo + rng.uniform(0.0, 0.2), ref, ref))
    order = rng.permutation(len(rows))                                  # the caller's order need not be the joints'
    return bodies, sid, joints, limits(*[rows[i] for i in order])


def test_device_matches_the_model_on_random_limited_joints():
    worst, differs = 0.0, 0
    for seed in range(30):
        bodies, sid, joints, lims = random_limited_scene(seed)
        want = jm.step(bodies, joints, lims, DT, 20)
        got = run_world(capi.SCENE_BOXES, bodies, sid, joints, lims, 1, 20)
        plain = jm.step(bodies, joints, NO_LIMITS, DT, 20)
        differs += np.abs(plain - want).max() > 1e-6                   # the limits bound
        worst = max(worst, np.abs(got - want).max())
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10, err_msg="seed %d" % seed)
    assert differs >= 25, differs
    print("largest |GPU - model| over 30 scenes: %.3g" % worst)


# ---- 4. sharded == single ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_sharded_world_with_limited_joints_across_cuts_equals_single(n_ranks):
    kind, n, substeps, frames = capi.SCENE_BOXES_DROP, 96, 6, 25
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 25:28] = np.random.default_rng(3).normal(scale=6.0, size=(n, 3))   # spinning: the limits bind
    joints = chain_joints(capi, n, every=1, distance=0.0, limit=n // 2)
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    joints["axis_a"] = joints["axis_b"] = Y
    hinges = np.arange(len(joints)) % 2 == 1
    joints["kind"][hinges] = capi.JOINT_HINGE
    rows = []
    for k in range(len(joints)):
        if hinges[k]:
            rows.append((k, capi.LIMIT_HINGE, -0.2, 0.3))
        else:
            rows += [(k, capi.LIMIT_TWIST, -0.1, 0.2), (k, capi.LIMIT_SWING, 0.0, 0.25)]
    lims = limits(*rows)
    one = run_world(kind, bodies, sid, joints, lims, frames, substeps)
    assert not bits_equal(one, run_world(kind, bodies, sid, joints, None, frames, substeps))
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        mw.set_joint_limits(lims)
        owner = mw.owners()
        for _ in range(frames):
            mw.step(DT, substeps)
        got = mw.download()
    crossing = owner[joints["body_a"]] != owner[joints["body_b"]]
    assert crossing.any()
    assert not np.isnan(one).any() and bits_equal(got, one)


def test_sharded_limits_set_before_the_first_step_and_upload_clears_them():
    kind, n, substeps, frames = capi.SCENE_BOXES_DROP, 64, 6, 10
    bodies, sid = line_scene(capi, kind, n, 4, 1.3)
    bodies[:, 25:28] = np.random.default_rng(5).normal(scale=3.0, size=(n, 3))
    joints = chain_joints(capi, n, every=1, distance=0.0, limit=n // 2)
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    joints["axis_a"] = joints["axis_b"] = Y
    lims = limits(*[(k, capi.LIMIT_SWING, 0.0, 0.1) for k in range(len(joints))])
    limited = run_world(kind, bodies, sid, joints, lims, frames, substeps)
    plain = run_world(kind, bodies, sid, joints, None, frames, substeps)
    assert not bits_equal(limited, plain)
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=2.0, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        mw.set_joint_limits(lims)
        for _ in range(frames):
            mw.step(DT, substeps)
        assert bits_equal(mw.download(), limited)
        mw.upload(bodies, sid, 0, n, joints)                            # clears the limits
        for _ in range(frames):
            mw.step(DT, substeps)
        assert bits_equal(mw.download(), plain)


# ---- 5. errors and clearing -------------------------------------------------------------------------------------------
def bad_limit_cases():
    """(name, limits) that xpbd_world_set_joint_limits must reject for the joints of door_and_ball()"""
    good_h = (0, capi.LIMIT_HINGE, -0.4, 0.6, X, X)
    cases = {
        "joint out of range": limits((2, capi.LIMIT_SWING, 0.0, 0.5)),
        "hinge limit on a ball joint": limits((1, capi.LIMIT_HINGE, -0.4, 0.6, Y, Y)),
        "swing limit on a hinge": limits((0, capi.LIMIT_SWING, 0.0, 0.5)),
        "twist limit on a hinge": limits((0, capi.LIMIT_TWIST, -0.3, 0.3, X, X)),
        "two of a kind": limits(good_h, good_h),
        "non-unit reference": limits((0, capi.LIMIT_HINGE, -0.4, 0.6, [2.0, 0.0, 0.0], X)),
        "reference along the axis": limits((0, capi.LIMIT_HINGE, -0.4, 0.6, X, Z)),
        "NaN bound": limits((0, capi.LIMIT_HINGE, float("nan"), 0.6, X, X)),
        "lower > upper": limits((0, capi.LIMIT_HINGE, 0.6, -0.4, X, X)),
        "bound beyond pi": limits((0, capi.LIMIT_HINGE, -0.4, 3.2, X, X)),
        "swing with lower != 0": limits((1, capi.LIMIT_SWING, 0.1, 0.5)),
        "unknown kind": limits((1, 7, 0.0, 0.5)),
    }
    return cases


def door_and_ball():
    """A hinged door (joint 0, limited to [-0.4, 0.6]) and a ball joint (joint 1, axes x) on two static posts."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 4)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 10:28] = 0.0
    for k, p in enumerate([[0, 0, 5], [2.5, 0, 5], [0, 6, 5], [2.5, 6, 5]]):
        bodies[k, 31:34] = p
    bodies[[0, 2], 0:10] = 0.0
    bodies[1, 27] = 20.0
    joints = np.zeros(2, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = [0, 2], [1, 3]
    joints["anchor_a"], joints["anchor_b"] = [2.0, 0.0, 0.5], [-0.5, 0.0, 0.5]
    joints["axis_a"][0] = joints["axis_b"][0] = Z
    joints["axis_a"][1] = joints["axis_b"][1] = X
    joints["kind"][0] = capi.JOINT_HINGE
    return bodies, sid, joints, limits((0, capi.LIMIT_HINGE, -0.4, 0.6, X, X))


def test_bad_limits_are_rejected_and_the_previous_ones_stay():
    bodies, sid, joints, good = door_and_ball()
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        w.set_joints(joints)
        for _ in range(30):
            w.step(DT, 20)
        free = w.download()
        w.upload(bodies, sid)
        w.set_joints(joints)
        w.set_joint_limits(good)
        for name, bad in bad_limit_cases().items():
            with pytest.raises(capi.XpbdError) as e:
                w.set_joint_limits(bad)
            assert e.value.code == capi.E_INVALID, name
        for _ in range(30):
            w.step(DT, 20)
        limited = w.download()
        assert bits_equal(limited, run_world(capi.SCENE_BOXES, bodies, sid, joints, good, 30, 20))   # `good` still acted
        assert not bits_equal(limited, free)
        # set_joints clears the limits, as does upload; an empty list clears them too
        for clear in ("set_joints", "upload", "empty"):
            w.upload(bodies, sid)
            w.set_joints(joints)
            w.set_joint_limits(good)
            if clear == "set_joints":
                w.set_joints(joints)
            elif clear == "upload":
                w.upload(bodies, sid)
                w.set_joints(joints)
            else:
                w.set_joint_limits(NO_LIMITS)
            for _ in range(30):
                w.step(DT, 20)
            assert bits_equal(w.download(), free), clear
    with capi.World(mode=capi.MODE_FUSED) as w:                         # only XPBD_MODE_CONTACTS takes limits
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        w.upload(bodies, sid)
        with pytest.raises(capi.XpbdError) as e:
            w.set_joint_limits(good)
        assert e.value.code == capi.E_INVALID


def test_multi_world_rejects_bad_limits_before_any_collective():
    bodies, sid, joints, good = door_and_ball()
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=0.75) as mw:
        mw.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        with pytest.raises(capi.XpbdError) as e:
            mw.set_joint_limits(good)                                   # no joints uploaded yet
        assert e.value.code == capi.E_INVALID
        mw.upload(bodies, sid, 0, len(bodies), joints)
        mw.set_joint_limits(good)
        for name, bad in bad_limit_cases().items():
            with pytest.raises(capi.XpbdError) as e:
                mw.set_joint_limits(bad)
            assert e.value.code == capi.E_INVALID, name
        for _ in range(30):
            mw.step(DT, 20)
        got = mw.download()
    assert bits_equal(got, run_world(capi.SCENE_BOXES, bodies, sid, joints, good, 30, 20))
