"""Kinematic bodies and island sleeping on the GPU (include/xpbd.h, "SLEEPING": a MOVING body is not inert and wakes what shares a
pair of the frame's pair list or a joint with it).

Two stacks of three boxes fall asleep, each on a kinematic slab of its own, 40 m apart.  One slab then becomes MOVING -- upwards
in one case, downwards (away from the stack: they stop touching in the first substep) in the other: after that frame's pass the
stack on it is awake, the other stack and its group are untouched.  The retarget itself wakes nobody; set_dynamics on the same
slab wakes both stacks, as before.  A sleeper that only a joint connects to a MOVING body wakes too.  After EVERY frame of every
run the asleep flags, counters, groups and the pass's counts equal tests/kinematic_sleep_model.py exactly."""
import numpy as np
import pytest

import islands_common as ic
import kinematic_common as kc
import kinematic_model as km
import kinematic_sleep_model as ksm
import sleep_common as sc
import sleep_model as sm
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

NO_JOINTS = ic.distance_joints([], [])


def sleeping_world(bodies, sid, joints, tbl):
    w = kc.new_world(bodies, sid, joints)
    w.set_contact_report(True)
    w.set_sleeping(*kc.SLEEP_CFG)
    w.set_kinematics(kc.to_capi(tbl))
    return w


def frames_against_model(w, joints, tbl, state, frames, where, requests=None):
    """Steps `frames` frames with `tbl` in force; after each the library's sleep state must equal the model's.  Returns (the
    frames, the model's state, who was MOVING in each frame)."""
    out, moved = [], []
    h = kc.DT / kc.SLEEP_SUBSTEPS
    for k in range(frames):
        _, moving = km.overwrite(w.download(), tbl, h, kc.SLEEP_SUBSTEPS)
        w.step(kc.DT, kc.SLEEP_SUBSTEPS)
        f = sc.Frame(w)
        pairs = ksm.pair_list(*w.frame_neighbours())
        if requests is None:                                            # rule (a): no pair with two inert ends
            inert = ksm.may_pair(state, f.bodies, moving)
            for a, b in pairs:
                assert not (inert[a] and inert[b]), (where, k, a, b)
        state, woken, slept = ksm.frame(state, f.bodies, f.pairs, joints, kc.SLEEP_CFG, moving, pairs, requests if k == 0 else None)
        sc.assert_state_equals_model(f, state, woken, slept, "%s, frame %d" % (where, k))
        out.append(f)
        moved.append(moving)
    return out, state, moved


def settled():
    """(world, model state, rows) of the two stacks asleep on their held slabs."""
    bodies, sid = kc.stacks_scene()
    tbl = kc.slab_tables(0.0, 1)[0]
    w = sleeping_world(bodies, sid, None, tbl)
    frames, state, moved = frames_against_model(w, NO_JOINTS, tbl, sm.State(w.n), kc.SETTLE_FRAMES, "settling")
    assert not np.any(moved)                                            # held slabs are not MOVING
    asleep = frames[-1].asleep
    assert all(asleep[i] for i in kc.STACK_A + kc.STACK_B) and not asleep[kc.SLAB_A] and not asleep[kc.SLAB_B]
    return w, state, frames[-1], tbl


@pytest.mark.parametrize("dz", [0.05, -0.05], ids=["upwards", "downwards"])
def test_a_moving_slab_wakes_the_stack_on_it_and_nobody_else(dz):
    w, state, rest, held = settled()
    with w:
        travel = kc.slab_tables(dz, 3)
        w.set_kinematic_targets(None, kc.rows_of(travel[0]))            # the retarget itself requests no wake
        assert bits_equal(w.sleep_state()[0], rest.asleep)
        frames, state, moved = frames_against_model(w, NO_JOINTS, travel[0], state, 1, "first frame of travel")
        assert moved[0][kc.SLAB_A] and not moved[0][kc.SLAB_B] and moved[0].sum() == 1
        f = frames[0]
        assert not any(f.asleep[i] for i in kc.STACK_A) and f.sleep_counts[2] == 3          # the stack on the MOVING slab woke
        for i in kc.STACK_B:                                            # the other stack: asleep, its group and its bits untouched
            assert f.asleep[i] and f.group[i] == rest.group[i] and bits_equal(f.bodies[i, sc.DYN], rest.bodies[i, sc.DYN])
        for i in kc.STACK_A:                                            # asleep during the frame: it moved only afterwards
            assert bits_equal(f.bodies[i, sc.DYN], rest.bodies[i, sc.DYN])
        assert abs(f.bodies[kc.SLAB_A, 33] - (2.0 + dz)) <= 4.0 * np.spacing(2.0 + abs(dz))
        for k in (1, 2):
            w.set_kinematic_targets(None, kc.rows_of(travel[k]))
            frames, state, _ = frames_against_model(w, NO_JOINTS, travel[k], state, 1, "travel frame %d" % k)
        moved_z = frames[0].bodies[kc.STACK_A[0], 33] - rest.bodies[kc.STACK_A[0], 33]
        assert moved_z * dz > 0.0                                       # awake now: the stack follows the slab, up or down
        frames, state, moved = frames_against_model(w, NO_JOINTS, travel[2], state, 3, "arrived")
        assert not np.any(moved)
        assert all(frames[-1].asleep[i] for i in kc.STACK_B)


def test_set_dynamics_on_the_slab_wakes_both_stacks():
    """The contrast (existing behaviour, unchanged): an edit that names a fixed body wakes everybody."""
    w, state, rest, held = settled()
    with w:
        row = w.get_dynamics([kc.SLAB_A])
        w.set_dynamics([kc.SLAB_A], row)
        frames, state, _ = frames_against_model(w, NO_JOINTS, held, state, 1, "after set_dynamics", requests=sm.Requests(bodies=[kc.SLAB_A]))
        assert frames[0].sleep_counts[0] == 0 and not frames[0].asleep.any()           # both stacks woke at the start of the frame
        assert frames[0].rest_frames[kc.STACK_B[0]] <= 1                # ... and their counters started over


def test_a_sleeper_jointed_to_a_moving_body_wakes():
    """The anchor and the box hanging 2 m below it share no pair (their spheres are apart): only the joint lane can wake it."""
    bodies, sid = kc.boxes(2, [[0.0, 0.0, 8.0], [0.0, 0.0, 6.0]], fixed=[0])
    joints = ic.distance_joints([0], [1], distance=2.0)
    held = km.table((0, km.POSE, [0.0, 0.0, 8.0], kc.IDENT))
    with sleeping_world(bodies, sid, joints, held) as w:
        frames, state, _ = frames_against_model(w, joints, held, sm.State(2), kc.SETTLE_FRAMES, "hanging")
        assert frames[-1].asleep[1] and not frames[-1].asleep[0]
        travel = km.table((0, km.POSE, [0.05, 0.0, 8.0], kc.IDENT))
        w.set_kinematic_targets(None, kc.rows_of(travel))
        frames, state, moved = frames_against_model(w, joints, travel, state, 1, "anchor moves")
        assert moved[0][0] and len(ksm.pair_list(*w.frame_neighbours())) == 0
        assert not frames[0].asleep[1] and frames[0].sleep_counts[2] == 1
        frames_against_model(w, joints, travel, state, 2, "afterwards")
