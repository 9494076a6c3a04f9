"""Island sleeping (xpbd_world_set_sleeping, _sleep_state, _wake_bodies; include/xpbd.h, "SLEEPING") on the GPU: against the
independent model (sleep_model.py) frame by frame, against a twin world that never sleeps, and against itself across history
and edits.  Every comparison is exact: integers equal, doubles bit-equal.

The stack scenes (sleep_common.stack_scene), measured with the CPU oracle (tests/oracle_binding.contacts_step, SAT, dt = 1/60,
20 substeps, pad 0.02) in a world that never sleeps; speeds in m/s and rad/s, the thresholds are 0.1 and 0.5:
  single box on the plane    8.1e-9 after frame 1, below 4e-14 from frame 2 on; angular speed below 1e-17
  3-stack, 2 mm gaps         frame 1: 0.1635 (the gaps close), frame 2: 0.1192, from frame 3 on: at most 0.0444 and 0.1905;
                             frames 30..60: at most 0.0179 and 0.1108
  box dropped from 5 m       its speed first falls in frame 61 (the landing); the 4-stack is at most 0.0613 and 0.4966 from frame
                             121 on, 0.0332 and 0.2304 from frame 201 on, 0.0280 and 0.1921 from frame 341 on
So the single box counts from frame 1 and sleeps in the pass of frame 30; the stack counts from frame 3 and sleeps in the pass
of frame 32; the dropped box lands about 30 frames after that."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import islands_common as ic
import islands_model as im
import sleep_common as sc
import sleep_model as sm
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DT, SUBSTEPS = sc.DT, sc.SUBSTEPS
NONE = capi.SLEEP_GROUP_NONE
U32_MAX = 0xFFFFFFFF


# ---- 1. off is the parent -------------------------------------------------------------------------------------------------------------
def test_a_world_that_never_sleeps_is_the_same_bits_with_sleeping_on_and_off():
    def run(variant):
        w, _ = ic.drop_world()
        out = []
        with w:
            if variant == "on_off":
                w.set_sleeping(*sc.LOOSE)
                w.set_sleeping()
            for k in range(30):
                if variant == "never" and k == 0:
                    w.set_sleeping(0.5, 2.0, U32_MAX)
                if variant == "on_off" and k == 10:
                    w.set_sleeping(0.5, 2.0, U32_MAX)
                if variant == "on_off" and k == 20:
                    w.set_sleeping()
                w.step(DT, 10)
                out.append(sc.Frame(w, state=False))
        return out
    off = run("off")
    assert off[-1].counts[0] > 0 and sum(len(f.events) for f in off) > 0    # boxes have begun to land on each other
    for variant in ("never", "on_off"):
        for k, (a, b) in enumerate(zip(off, run(variant))):
            assert im.same_bytes(a.bodies, b.bodies), (variant, k)
            assert a.counts == b.counts, (variant, k, a.counts, b.counts)
            assert im.same_bytes(a.events, b.events) and im.same_bytes(a.pairs, b.pairs), (variant, k)
            assert im.same_bytes(a.contacts, b.contacts), (variant, k)


# ---- 2 - 6. the stack scenes and the crafted scene: one run each, with the model beside it and a twin that never sleeps ----------------
run_with_twin = sc.run_with_twin


@pytest.fixture(scope="module")
def stack_run():
    return run_with_twin(lambda on: sc.stack_world(False, sc.CFG if on else None), 120)


@pytest.fixture(scope="module")
def dropper_run():
    return run_with_twin(lambda on: sc.stack_world(True, sc.CFG if on else None), 450)


@pytest.fixture(scope="module")
def crafted_run():
    return run_with_twin(lambda on: sc.crafted_world(sc.CFG if on else None), 120)


def first_asleep(frames, body):
    """1-based frame whose pass put the body to sleep first, or None."""
    for k, f in enumerate(frames):
        if f.asleep[body]:
            return k + 1
    return None


def test_stacks_sleep(stack_run):
    frames, _ = stack_run
    print("asleep first: single %s, stack %s" % (first_asleep(frames, sc.SINGLE), [first_asleep(frames, b) for b in sc.STACK]))
    assert first_asleep(frames, sc.SINGLE) == 30             # at rest from frame 1: asleep after exactly 30 frames
    assert frames[29].group[sc.SINGLE] == sc.SINGLE and frames[29].rest_frames[sc.SINGLE] == 30
    at = {first_asleep(frames, b) for b in sc.STACK}
    assert len(at) == 1                                      # as one island
    (k,) = at
    assert k is not None and 30 <= k <= 60
    assert all(frames[59].group[b] == 0 and frames[59].asleep[b] for b in sc.STACK)
    assert first_asleep(frames, sc.FALLING) is None          # 120 frames of free fall from 50 m
    assert frames[59].sleep_counts[:2] == (4, 2)


def test_touch_wakes(dropper_run):
    frames, _ = dropper_run
    slept_at = first_asleep(frames, 0)
    touch = next(k + 1 for k, f in enumerate(frames)
                 if any(int(p["body_b"]) == sc.DROPPER and int(p["body_a"]) in sc.STACK for p in f.pairs))
    print("stack asleep in frame %s, first pair with the dropped box in frame %d" % (slept_at, touch))
    assert slept_at is not None and slept_at < touch
    before, at = frames[touch - 2], frames[touch - 1]
    assert all(before.asleep[b] for b in sc.STACK)
    assert not any(at.asleep[b] for b in sc.STACK) and at.sleep_counts[2] == 3          # the whole group, in that frame's pass
    assert all(at.group[b] == NONE for b in sc.STACK)
    again = [first_asleep(frames[touch:], b) for b in sc.STACK + (sc.DROPPER,)]
    print("asleep again %s frames after the touch" % again)
    assert all(frames[-1].asleep[b] and frames[-1].group[b] == 0 for b in sc.STACK + (sc.DROPPER,))
    # BEGIN events when the group wakes: the pairs inside it are back in the report
    woke_pairs = {(int(p["body_a"]), int(p["body_b"])) for p in at.pairs}
    assert (2, sc.DROPPER) in woke_pairs
    after = frames[touch]
    begins = {(int(e["body_a"]), int(e["body_b"])) for e in after.events if e["kind"] == capi.CONTACT_BEGIN}
    assert {(0, 1), (1, 2)} <= begins


@pytest.mark.parametrize("run", ["stack_run", "dropper_run", "crafted_run"])
def test_frozen_while_asleep(run, request):
    frames, _ = request.getfixturevalue(run)
    assert sc.assert_frozen(frames) > 100


@pytest.mark.parametrize("run,far", [("stack_run", (sc.FALLING,)), ("dropper_run", (sc.FALLING,)), ("crafted_run", (10, 11, 12, 13, 14, 15))])
def test_exact_twin(run, far, request):
    """Until the first island sleeps everything is the twin's bits.  After that a body more than 10 m from all others, which has
    no pair with a sleeper, stays the twin's bits for as long as it has been awake since the start.
    NOT compared here: an awake body that touches a sleeper -- the twin's partner moves, so there is no twin to compare with.  That
    body is held to the extended-precision model by test_gpu_xprec_sleep.py."""
    frames, twin = request.getfixturevalue(run)
    assert sc.assert_twin(frames, twin, far) >= 120          # (the falling box alone gives that many)


@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
def test_box_drop_equals_the_model_every_frame(narrowphase):
    """Loose thresholds: many groups fall asleep while their neighbours still move, and are woken again."""
    w, joints = sc.drop_world(narrowphase)
    with w:
        frames, state = sc.run_against_model(w, joints, sc.LOOSE, 120, substeps=10)
    slept = sum(f.sleep_counts[3] for f in frames)
    woken = sum(f.sleep_counts[2] for f in frames)
    print("put to sleep %d, woken %d, asleep at the end %d in %d groups" % ((slept, woken) + frames[-1].sleep_counts[:2]))
    assert slept > 100 and woken > 0 and frames[-1].sleep_counts[1] > 1
    assert not state.asleep[5] and not state.asleep[200]     # the fixed bodies never sleep


# ---- 7. edits wake --------------------------------------------------------------------------------------------------------------------
QUICK = (0.1, 0.5, 5)


class Edit(sm.Requests):
    def __init__(self, apply, bodies=(), wake_all=False, zero_counters=False):
        super().__init__(bodies, wake_all, zero_counters)
        self.apply = apply


def body_edits(bodies):
    """Each names body 1 (in the stack 0-2) without changing anything a step reads."""
    return {
        "wake_bodies": Edit(lambda w: w.wake_bodies([1]), [1]),
        "set_external_wrench": Edit(lambda w: w.set_external_wrench([1], force=bodies[1, 10:13].reshape(1, 3)), [1]),
        "apply_impulses": Edit(lambda w: w.apply_impulses(capi.impulses([1], np.zeros((1, 3)))), [1]),
        "set_dynamics": Edit(lambda w: w.set_dynamics([1], w.get_dynamics([1])), [1]),
    }


def table_edits(joints):
    return {
        "set_joints": lambda w: w.set_joints(joints),
        "set_joint_limits": lambda w: w.set_joint_limits(np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE)),
        "set_joint_drives": lambda w: w.set_joint_drives(np.zeros(0, dtype=capi.JOINT_DRIVE_DTYPE)),
        "set_collision_filters": lambda w: w.set_collision_filters(),
        "set_materials": lambda w: w.set_materials(),
        "set_restitution": lambda w: w.set_restitution(),
        "set_terrain": lambda w: w.set_terrain(),
        "set_polytopes": lambda w: w.set_polytopes([capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, ic.SLAB)]),
        "set_contact_pad": lambda w: w.set_contact_pad(0.02),
    }


def test_edits_wake_their_group_and_table_setters_wake_all():
    w, joints = sc.crafted_world(QUICK)
    with w:
        bodies = w.download()
        frames, state = sc.run_against_model(w, joints, QUICK, 12)
        at = 13
        assert all(state.asleep[i] for i in (0, 1, 2, 3, 4, 5)) and state.group[1] == 0 and state.group[4] == 3
        for name, edit in body_edits(bodies).items():
            frames, state = sc.run_against_model(w, joints, QUICK, 1, requests={at: edit}, state=state, first_frame=at)
            assert not any(state.asleep[i] for i in (0, 1, 2)), name              # its group
            assert all(state.asleep[i] for i in (3, 4, 5)), name                  # and no other
            assert state.rest_frames[1] == 1 and state.rest_frames[4] >= 5, name  # woken at the start of the frame, counted at its end
            frames, state = sc.run_against_model(w, joints, QUICK, 8, state=state, first_frame=at + 1)
            assert all(state.asleep[i] for i in (0, 1, 2)), name
            at += 9
        # an edit that names a fixed body: everybody wakes
        slab = Edit(lambda w: w.set_dynamics([6], w.get_dynamics([6])), [6])
        frames, state = sc.run_against_model(w, joints, QUICK, 1, requests={at: slab}, state=state, first_frame=at)
        assert frames[-1].sleep_counts[0] == 0
        frames, state = sc.run_against_model(w, joints, QUICK, 8, state=state, first_frame=at + 1)
        at += 9
        for name, apply in table_edits(joints).items():
            assert all(state.asleep[i] for i in (0, 1, 2, 3, 4, 5)), name
            frames, state = sc.run_against_model(w, joints, QUICK, 1, requests={at: Edit(apply, wake_all=True, zero_counters=True)}, state=state,
                                                 first_frame=at)
            assert frames[-1].sleep_counts[0] == 0 and int(frames[-1].rest_frames.max()) <= 1, name
            frames, state = sc.run_against_model(w, joints, QUICK, 8, state=state, first_frame=at + 1)
            at += 9
        w.wake_bodies()
        frames, state = sc.run_against_model(w, joints, QUICK, 1, requests={at: sm.Requests(wake_all=True)}, state=state, first_frame=at)
        assert frames[-1].sleep_counts[0] == 0


@pytest.fixture(scope="module")
def device_child(tmp_path_factory):
    """sleep_device_child.py, once: the device variants driven from torch tensors on a torch stream, beside the host variants."""
    out = tmp_path_factory.mktemp("sleeping") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "sleep_device_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out)), json.loads(p.stdout.strip().splitlines()[-1])


def test_device_variants_give_the_host_variants_state(device_child):
    res, verdict = device_child
    assert verdict["steps"] >= 4
    for k in range(verdict["steps"]):
        for what in ("asleep", "rest_frames", "group", "counts", "bodies"):
            assert im.same_bytes(res["host_%d_%s" % (k, what)], res["device_%d_%s" % (k, what)]), (k, what)
        assert im.same_bytes(res["device_%d_asleep" % k], res["device_%d_dev_asleep" % k])           # xpbd_world_sleep_state_device
        assert im.same_bytes(res["device_%d_rest_frames" % k], res["device_%d_dev_rest_frames" % k])
        assert im.same_bytes(res["device_%d_group" % k], res["device_%d_dev_group" % k])
        assert im.same_bytes(res["device_%d_counts" % k], res["device_%d_dev_counts" % k])
    for k in verdict["woke_stack"]:
        assert not res["device_%d_asleep" % k][:3].any() and res["device_%d_asleep" % k][3:6].all(), k
    for k in verdict["woke_all"]:
        assert not res["device_%d_asleep" % k].any(), k


# ---- 8. history and population --------------------------------------------------------------------------------------------------------
def test_history_restores_the_sleep_state_and_the_run():
    w, joints = sc.crafted_world(QUICK)
    with w:
        sc.run_against_model(w, joints, QUICK, 10)
        assert w.sleep_state()[3][0] >= 6
        w.wake_bodies([4])                                   # a request pending at the push travels with it
        index = w.history_push()

        def record():
            out = []
            for _ in range(20):
                w.step(DT, SUBSTEPS)
                out.append(sc.Frame(w))
            return out
        first = record()
        assert not first[0].asleep[3:6].any() and first[0].asleep[0:3].all()
        w.history_restore(index)
        restored = w.sleep_state()
        assert restored[0][3:6].all() and restored[3][0] >= 6
        second = record()
        for k, (a, b) in enumerate(zip(first, second)):
            assert im.same_bytes(a.bodies, b.bodies), k
            assert im.same_bytes(a.asleep, b.asleep) and im.same_bytes(a.rest_frames, b.rest_frames) and im.same_bytes(a.group, b.group), k
            assert a.sleep_counts == b.sleep_counts and im.same_bytes(a.contacts, b.contacts), k
        # turning sleeping off changes the size of an entry: the history goes
        assert w.history_length() == 1
        w.set_sleeping()
        assert w.history_length() == 0


def test_population_change_wakes_all_and_steps_like_a_fresh_world():
    w, joints = sc.crafted_world(QUICK)
    with w:
        sc.run_against_model(w, joints, QUICK, 10)
        assert w.sleep_state()[3][0] >= 6
        extra, _ = capi.scene_generate(ic.BOXES, 5, 1)
        extra[:, 22:28] = 0.0
        extra[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
        extra[:, 31:34] = [60.0, 0.0, 0.0]
        w.add_bodies(extra, np.zeros(1, dtype=np.uint32))
        asleep, rest, group, counts = w.sleep_state()
        assert not asleep.any() and not rest.any() and np.all(group == NONE) and counts == (0, 0, 0, 0)
        bodies = w.download()
        fresh = capi.World(mode=capi.MODE_CONTACTS)
        with fresh:
            fresh.set_polytopes([capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, ic.SLAB)])
            sid = np.zeros(17, dtype=np.uint32)
            sid[6] = 1
            fresh.upload(bodies, sid)
            fresh.set_joints(joints)
            fresh.set_contact_report(True)
            fresh.set_sleeping(*QUICK)
            state = sm.State(17)
            for k in range(15):
                w.step(DT, SUBSTEPS)
                fresh.step(DT, SUBSTEPS)
                a, b = sc.Frame(w), sc.Frame(fresh)
                assert im.same_bytes(a.bodies, b.bodies), k
                assert im.same_bytes(a.asleep, b.asleep) and im.same_bytes(a.rest_frames, b.rest_frames) and im.same_bytes(a.group, b.group), k
                state, woken, slept = sm.frame(state, a.bodies, a.pairs, joints, QUICK)
                sc.assert_state_equals_model(a, state, woken, slept, "frame %d after the change" % (k + 1))
            assert state.asleep[16] and state.asleep[0:6].all()
        # a removal starts the state over as well
        w.remove_bodies([16])
        assert not w.sleep_state()[0].any()
        # and so does an upload
        for _ in range(8):
            w.step(DT, SUBSTEPS)
        assert w.sleep_state()[0].any()
        w.upload(bodies[:16], sid[:16])
        w.set_joints(joints)
        w.set_contact_report(True)
        assert not w.sleep_state()[0].any() and w.sleep_state()[1].max() == 0


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def test_every_invalid_call_is_refused_with_nothing_written():
    L = capi.hip_lib()
    E = capi.E_INVALID

    def cfg(lin=0.1, ang=0.5, frames=30, flags=0):
        return C.byref(capi.SLEEP_CONFIG(lin, ang, frames, flags))
    assert L.xpbd_world_set_sleeping(None, cfg()) == E
    w, _ = sc.stack_world(sleeping=None)
    with w:
        h = w._h
        for bad in (cfg(lin=-1.0), cfg(lin=np.inf), cfg(lin=np.nan), cfg(ang=-0.5), cfg(ang=np.inf), cfg(ang=np.nan), cfg(frames=0), cfg(flags=1)):
            assert L.xpbd_world_set_sleeping(h, bad) == E
        sentinel = np.full(w.n, 0x5A, dtype=np.uint8)
        counts = (C.c_uint32 * 4)(7, 7, 7, 7)
        # sleeping off: the state and wake calls
        assert L.xpbd_world_sleep_state(h, sentinel.ctypes.data, None, None, counts) == E
        assert np.all(sentinel == 0x5A) and list(counts) == [7, 7, 7, 7]
        assert L.xpbd_world_sleep_state_device(h, None, None, None, None) == E
        assert L.xpbd_world_wake_bodies(h, None, 0) == E and L.xpbd_world_wake_bodies_device(h, None, 0) == E
        assert L.xpbd_world_sleep_state(None, None, None, None, None) == E and L.xpbd_world_wake_bodies(None, None, 0) == E
        # the report off, another mode
        w.set_contact_report(False)
        assert L.xpbd_world_set_sleeping(h, cfg()) == E
        w.set_contact_report(True)
        w.set_mode(capi.MODE_FUSED)
        assert L.xpbd_world_set_sleeping(h, cfg()) == E
        w.set_mode(capi.MODE_CONTACTS)
        for _ in range(3):
            w.step(DT, SUBSTEPS)
        before = w.download()
        assert L.xpbd_world_sleep_state(h, None, None, None, None) == E          # none of the refusals turned it on
        w.set_sleeping(*sc.CFG)
        # while it is on
        assert L.xpbd_world_set_contact_report(h, 0) == E
        assert L.xpbd_world_set_mode(h, capi.MODE_FUSED) == E and L.xpbd_world_set_mode(h, capi.MODE_PER_SUBSTEP) == E
        assert L.xpbd_world_contacts_begin(h, C.c_double(DT)) == E and L.xpbd_world_contacts_substep(h, C.c_double(DT / 20)) == E
        entries = C.c_uint32(7)
        assert L.xpbd_world_build_neighbours(h, C.c_double(DT), C.byref(entries)) == E and entries.value == 7   # a broadphase outside a step
        idx = np.array([1, w.n], dtype=np.uint32)
        assert L.xpbd_world_wake_bodies(h, idx.ctypes.data, 2) == E              # an index out of range
        assert L.xpbd_world_wake_bodies(h, None, 3) == E and L.xpbd_world_wake_bodies_device(h, None, 3) == E
        assert L.xpbd_world_set_sleeping(h, cfg(frames=0)) == E                  # and the configuration in force stays
        assert im.same_bytes(before, w.download())
        w.set_contact_report(True)                                               # enabling again is allowed
        w.step(DT, SUBSTEPS)
        assert w.sleep_state()[3] == (0, 0, 0, 0)
        w.set_sleeping()
        w.set_contact_report(False)
        w.set_mode(capi.MODE_FUSED)
