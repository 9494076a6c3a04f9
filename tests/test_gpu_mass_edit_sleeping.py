"""Mass edits and island sleeping on the GPU (include/xpbd.h, "MASS properties of resident bodies": SLEEPING).

Two stacks of three boxes, 20 m apart, fall asleep; a fixed box hovers far from both.  A mass edit is an edit: naming a sleeper
wakes its group at the start of the next step, naming a fixed body wakes everybody -- judged by the mass properties from BEFORE
the edit, because the wake requests are enqueued before the edit kernel.  After EVERY frame of every run the asleep flags, counters,
groups and the pass's counts equal the model exactly: tests/sleep_model.py, whose frame tests/mass_edit_model.py restates with the
request judged before the edit and the pass run on the bodies after it."""
import numpy as np
import pytest

import islands_common as ic
import islands_model as im
import mass_edit_common as mc
import mass_edit_model as mm
import sleep_common as sc
import sleep_model as sm
from constraint_solver_amd import capi
from mass_edit_common import same

pytestmark = pytest.mark.gpu

NO_JOINTS = ic.distance_joints([], [])
A, B = list(mc.STACK_A), list(mc.STACK_B)


def frames_against_model(w, state, frames, where, named=(), fixed_when_named=None):
    """Steps `frames` frames; after each the library's sleep state must equal the model's.  named / fixed_when_named: the bodies
    an edit named since the last frame and who was fixed when it did.  Returns (the frames, the model's state)."""
    out = []
    for k in range(frames):
        w.step(mc.DT, mc.SUBSTEPS)
        f = sc.Frame(w)
        state, woken, slept = mm.sleep_frame(state, f.bodies, f.pairs, NO_JOINTS, mc.SLEEP_CFG, named if k == 0 else (), fixed_when_named)
        sc.assert_state_equals_model(f, state, woken, slept, "%s, frame %d" % (where, k))
        out.append(f)
    return out, state


def settled():
    """(world, model state, last frame) of the two stacks asleep."""
    w = mc.stacks_world()
    frames, state = frames_against_model(w, sm.State(w.n), mc.SETTLE_FRAMES, "settling")
    asleep = frames[-1].asleep
    assert asleep[A + B].all() and not asleep[mc.ANCHOR]
    assert len({int(g) for g in frames[-1].group[A]}) == 1 and frames[-1].group[A[0]] != frames[-1].group[B[0]]
    return w, state, frames[-1]


def edit(w, body, change, flags=mm.INVERSE):
    """One body re-weighed by change(row): (who was fixed before the call, the row it had)."""
    fixed = im.fixed_bodies(w.download())
    saved = w.get_mass_properties([body])
    row = saved.copy()
    change(row[0])
    w.set_mass_properties([body], row, flags)
    return fixed, saved


def heavier(row):
    row[0:10] /= 10.0


def frozen(row):
    row[0:10] = 0.0


def test_reweighing_a_sleeper_wakes_its_group_in_the_next_frame_and_nobody_else():
    w, state, rest = settled()
    with w:
        fixed, _ = edit(w, A[0], heavier)
        assert same(w.sleep_state()[0], rest.asleep)                      # nothing wakes before the next step
        frames, state = frames_against_model(w, state, 1, "re-weighed", [A[0]], fixed)
        f = frames[0]
        assert not f.asleep[A].any()                                     # only its group woke, in the next frame
        assert f.asleep[B].all() and same(f.group[B], rest.group[B]) and same(f.bodies[B][:, sc.DYN], rest.bodies[B][:, sc.DYN])
        frames, state = frames_against_model(w, state, mc.SLEEP_CFG[2] + 4, "afterwards")
        assert frames[-1].asleep[A + B].all()                            # it rests again, ten times heavier


def test_naming_a_fixed_body_wakes_everybody():
    w, state, rest = settled()
    with w:
        fixed, _ = edit(w, mc.ANCHOR, lambda row: None)                  # the same row again: an anchor was named
        frames, state = frames_against_model(w, state, 1, "anchor named", [mc.ANCHOR], fixed)
        assert not frames[0].asleep.any() and frames[0].rest_frames[A + B].max() <= 1
        frames_against_model(w, state, 3, "afterwards")


def test_freezing_the_middle_sleeper_splits_the_stack_and_releasing_it_wakes_all():
    w, state, rest = settled()
    with w:
        # (c) the middle sleeper becomes fixed: its group wakes, it is inert and never asleep again, what lies on it sleeps anchored
        fixed, saved = edit(w, mc.MIDDLE, frozen)
        assert not fixed[mc.MIDDLE]
        frames, state = frames_against_model(w, state, 1, "frozen", [mc.MIDDLE], fixed)
        assert not frames[0].asleep[A].any() and frames[0].asleep[B].all() and same(frames[0].group[B], rest.group[B])
        # 8. the islands after (c), while the group is awake: the 3-stack has split, the new fixed body is no member, and each of
        # its neighbours counts it as an anchor
        island_of, records = ic.assert_equals_model(w, NO_JOINTS, 0)
        assert island_of[mc.MIDDLE] == capi.ISLAND_NONE and island_of[A[0]] != island_of[A[2]]
        assert records["n_anchors"][island_of[A[0]]] == 1 and records["n_anchors"][island_of[A[2]]] == 1
        more, state = frames_against_model(w, state, mc.SLEEP_CFG[2] + 4, "frozen, later")
        for f in frames + more:
            assert not f.asleep[mc.MIDDLE] and f.rest_frames[mc.MIDDLE] == 0
            # it went to sleep with velocities of +0.0, so it stays put (the integrate stage still renormalises its rotation)
            assert np.abs(f.bodies[mc.MIDDLE, 31:38] - rest.bodies[mc.MIDDLE, 31:38]).max() <= 1e-12 and np.abs(f.bodies[mc.MIDDLE, 22:28]).max() <= 1e-9
        last = more[-1]
        assert last.asleep[A[0]] and last.asleep[A[2]] and last.group[A[0]] != last.group[A[2]]   # two groups now, each anchored
        assert last.asleep[B].all() and same(last.group[B], rest.group[B])
        # ... and once they sleep again (a pair of a sleeper and a fixed body has two inert ends: the broadphase drops it, the
        # report and the model with it)
        island_of, records = ic.assert_equals_model(w, NO_JOINTS, 0)
        assert island_of[mc.MIDDLE] == capi.ISLAND_NONE and island_of[A[0]] != island_of[A[2]]
        # (d) release: a fixed body was named, so everybody wakes
        now_fixed = im.fixed_bodies(w.download())
        assert now_fixed[mc.MIDDLE]
        w.set_mass_properties([mc.MIDDLE], saved)
        assert same(w.get_mass_properties([mc.MIDDLE]), saved)
        frames, state = frames_against_model(w, state, 1, "released", [mc.MIDDLE], now_fixed)
        assert not frames[0].asleep.any()
        frames, state = frames_against_model(w, state, mc.SLEEP_CFG[2] + 4, "released, later")
        assert frames[-1].asleep[A + B].all() and len({int(g) for g in frames[-1].group[A]}) == 1
