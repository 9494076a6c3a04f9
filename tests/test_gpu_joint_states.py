"""Joint states and drive targets on the GPU (include/xpbd.h, "Joint STATES and drive TARGETS").

Joint states: the device agrees with the independent model (tests/joint_state_model.py) on random assembled mechanisms of every
joint, limit and drive kind after a few frames of stepping -- joint, kind and flags exactly, the eight doubles to a measured
tolerance -- in worlds of 1, 65 and 257 joints; a subset call gives the rows of the all-joints call, the device variant the host
variant's bits, an index out of range its 0xFFFFFFFF record with the neighbours intact; and asking changes nothing: the world
and its next 10 frames equal a twin that never asked.

Drive targets, each once with the eight-lane and once with the one-lane pair solve, all bit for bit: a host retarget equals a
twin given the whole table with the new targets; the device variant equals the host variant; a device call with invalid
entries equals a world given only the valid ones, and the host variant refuses the same list and then steps like an untouched
twin; after a device retarget, a population change and a SLIDE-limit change keep the new targets.  With sleeping on, a retarget
wakes the groups it touches and nobody else.  A control loop that stays on the device agrees with the same loop through the
CPU model.

TOLERANCE.  The largest |device - model| over all eight doubles of every joint of every world of the first test was measured on
an MI355X (printed by the test; the figure is in DESIGN.md 8, "Joint states and drive targets"); the test asserts 16 times
that, and never more than 1e-10, the bound the project asserts for whole driven runs against these models."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import joint_drive_model as jd
import joint_state_common as jc
import joint_state_model as jsm
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = 2.49e-14           # largest |device - model| on the MI355X (the 257-joint world; 1 joint: 1.33e-15, 65 joints: 6.38e-15)
TOLERANCE = min(16 * MEASURED, 1e-10)


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """joint_state_device_child.py, once: the device variants driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("joint_states") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "joint_state_device_child.py"), str(out)], capture_output=True, text=True, timeout=600)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):       # killed: nothing more is started on that GPU
        pytest.exit("joint_state_device_child.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["runs"] > 20
    return dict(np.load(out))


# ---- joint states -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints,seeds", [(1, range(jc.N_RECIPES))] + [(n, [0]) for n in jc.STATE_WORLDS])
def test_states_match_the_model(n_joints, seeds):
    worst = 0.0
    for seed in seeds:
        w, (bodies, sid, joints, lims, drvs) = jc.stepped_world(n_joints, seed)
        with w:
            rows, got = w.download(), w.joint_states()
        want, margin = jsm.joint_states(rows, joints, lims, drvs)
        assert margin >= 1e-6, (n_joints, seed, margin)                # no limit bit hinges on rounding
        for name in ("joint", "kind", "flags", "reserved"):
            assert np.array_equal(got[name], want[name]), (n_joints, seed, name, np.flatnonzero(got[name] != want[name])[:8])
        for name in jsm.DOUBLES:
            diff = np.abs(got[name] - want[name]).max()
            worst = max(worst, diff)
            assert diff <= TOLERANCE, (n_joints, seed, name, diff)
        for name, flag in (("angle", jsm.HAS_ANGLE), ("angle_rate", jsm.HAS_ANGLE), ("travel", jsm.HAS_TRAVEL), ("travel_rate", jsm.HAS_TRAVEL),
                           ("swing", jsm.HAS_SWING), ("twist", jsm.HAS_TWIST)):
            off = (got["flags"] & flag) == 0                            # a field that is not available is +0.0
            assert not got[name][off].view(np.uint64).any(), (n_joints, seed, name)
        assert not got["misalignment"][got["kind"] == capi.JOINT_DISTANCE].view(np.uint64).any()
    print("%d joint(s): largest |device - model| %.3g (asserted: %.3g)" % (n_joints, worst, TOLERANCE))


def test_asking_changes_nothing_and_a_subset_is_the_same_rows():
    n = jc.STATE_WORLDS[0]
    w, scene = jc.stepped_world(n, 0)
    twin, _ = jc.stepped_world(n, 0)
    with w, twin:
        everybody = w.joint_states()
        subset = np.array([n - 1, 3, 17, 3, 0], dtype=np.uint32)
        assert same_records(w.joint_states(subset), everybody[subset])
        assert same_records(w.joint_states(np.arange(n)), everybody) and same_records(w.joint_states(), everybody)
        assert len(w.joint_states([])) == 0
        assert bits_equal(w.download(), twin.download())
        for frame in range(10):
            w.step(jc.DT, jc.SUBSTEPS)
            twin.step(jc.DT, jc.SUBSTEPS)
            w.joint_states()
            assert bits_equal(w.download(), twin.download()), frame
        # the refusals that need a live world: nothing is written
        before = np.full(160, 0x5A, dtype=np.uint8).view(capi.JOINT_STATE_DTYPE)
        out = before.copy()
        L = capi.hip_lib()
        bad = np.array([1, n], dtype=np.uint32)
        assert L.xpbd_world_joint_states(w._h, bad.ctypes.data, 2, out.ctypes.data) == capi.E_INVALID
        assert L.xpbd_world_joint_states(w._h, None, n - 1, out.ctypes.data) == capi.E_INVALID
        assert L.xpbd_world_joint_states(w._h, bad.ctypes.data, 2, None) == capi.E_INVALID
        assert same_records(out, before)
    with capi.World(mode=capi.MODE_FUSED) as empty:                     # every mode; a world without joints accepts n == 0
        empty.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
        assert len(empty.joint_states()) == 0
        empty.set_drive_targets(None, [])


def test_states_device_variant_gives_the_host_variants_bits(child):
    assert len(child["states_host_all"]) == jc.STATE_WORLDS[0]
    assert same_records(child["states_device_all"], child["states_host_all"])
    assert same_records(child["states_device_subset"], child["states_host_subset"])
    assert same_records(child["states_host_subset"], child["states_host_all"][child["states_subset"]])


def test_states_device_variant_marks_an_index_out_of_range(child):
    got, asked, everybody = child["states_device_outside"], child["states_outside"], child["states_host_all"]
    guard = np.full(80, 0x5A, dtype=np.uint8).view(capi.JOINT_STATE_DTYPE)
    no_joint = np.zeros(1, dtype=capi.JOINT_STATE_DTYPE)
    no_joint["kind"] = capi.JOINT_STATE_NO_JOINT
    assert same_records(got[:1], guard) and same_records(got[-1:], guard)   # nothing outside the call's records
    for k, joint in enumerate(asked):
        want = everybody[joint:joint + 1] if joint < len(everybody) else no_joint
        assert same_records(got[1 + k:2 + k], want), (k, joint)


# ---- drive targets ----------------------------------------------------------------------------------------------------
SIZES = [pytest.param(False, id="eight_lanes"), pytest.param(True, id="one_lane")]
_RUNS = {}


def run(key, big, retarget, drives, targets):
    if (key, big) not in _RUNS:
        _RUNS[key, big] = jc.retarget_run(retarget, big, drives, targets)
    return _RUNS[key, big]


def drives_of_the_scene():
    return jc.driven_scene(False)[4]


def untouched(big):
    return run("untouched", big, lambda w, drives, targets: None, None, None)


@pytest.mark.parametrize("big", SIZES)
def test_host_retarget_equals_the_whole_table_with_the_new_targets(big):
    drvs = drives_of_the_scene()
    assert {int(k) for k in drvs["kind"]} == {0, 1, 2, 3}
    everybody = jc.new_targets(drvs)
    got = run("host_all", big, jc.host_retarget, None, everybody)
    assert bits_equal(got, run("table_all", big, jc.table_retarget(drvs), None, everybody))
    assert not bits_equal(got, untouched(big))                          # (the new targets do act)
    some, targets = jc.some_drives(drvs)
    got = run("host_some", big, jc.host_retarget, some, targets)
    assert bits_equal(got, run("table_some", big, jc.table_retarget(drvs), some, targets))
    assert not bits_equal(got, run("host_all", big, jc.host_retarget, None, everybody)) and not bits_equal(got, untouched(big))


@pytest.mark.parametrize("big", SIZES)
def test_device_retarget_equals_the_host_retarget(big, child):
    drvs = drives_of_the_scene()
    tag = "big_" if big else "small_"
    assert bits_equal(child[tag + "all"], run("host_all", big, jc.host_retarget, None, jc.new_targets(drvs)))
    assert bits_equal(child[tag + "some"], run("host_some", big, jc.host_retarget, *jc.some_drives(drvs)))


@pytest.mark.parametrize("big", SIZES)
def test_invalid_entries_are_skipped_on_the_device_and_refused_by_the_host(big, child):
    drvs = drives_of_the_scene()
    drives, targets, valid = jc.invalid_list(drvs)
    only_valid = run("valid_only", big, jc.host_retarget, drives[valid], targets[valid])
    assert bits_equal(child[("big_" if big else "small_") + "invalid"], only_valid)
    assert not bits_equal(only_valid, untouched(big))

    def refused(w, drives, targets):
        with pytest.raises(capi.XpbdError) as e:
            w.set_drive_targets(drives, targets)
        assert e.value.code == capi.E_INVALID
    assert bits_equal(run("refused", big, refused, drives, targets), untouched(big))


@pytest.mark.parametrize("change", ["remove", "slide"])
@pytest.mark.parametrize("big", SIZES)
def test_targets_set_on_the_device_survive_a_restaging_of_the_tables(big, change, child):
    tag = ("big_" if big else "small_") + change
    assert bits_equal(child[tag + "_kept"], child[tag + "_fresh"])
    assert not np.isnan(child[tag + "_kept"]).any()


def test_host_targets_survive_a_restaging_too():
    """... as they always did through the host copy: the host variant keeps it true itself."""
    bodies, sid, joints, lims, drvs, n_mech = jc.driven_scene(False, extra_bodies=1)
    targets = jc.new_targets(drvs)
    table = drvs.copy()
    table["target"] = targets
    with jc.new_world(bodies, sid, joints, lims, drvs) as w, jc.new_world(bodies, sid, joints, lims, table) as t:
        w.set_drive_targets(None, targets)
        for world in (w, t):
            world.remove_bodies([n_mech - 1])
            for _ in range(jc.RETARGET_THEN):
                world.step(jc.DT, jc.SUBSTEPS)
        assert bits_equal(w.download(), t.download())


# ---- sleeping ---------------------------------------------------------------------------------------------------------
def test_a_retarget_wakes_the_groups_it_touches_and_nobody_else(child):
    w, drvs = jc.sleeping_world()
    with w:
        asleep = jc.wake_sequence(w, drvs, jc.host_retarget).astype(bool)
    settled, fixed_base, first, table = asleep
    print("asleep after settling / retarget on the fixed base / retarget of mechanism 0 / set_joint_drives:", asleep.astype(int).tolist())
    assert settled.tolist() == [True, True, True, True, False, True]    # everybody but the fixed base
    assert fixed_base.tolist() == [True, True, True, True, False, False]   # its free end wakes; the fixed end asks for nothing more
    assert first[:2].tolist() == [False, False] and first[2:4].tolist() == [True, True]   # mechanism 0 wakes, mechanism 1 sleeps on
    assert not table.any()                                              # the whole table wakes every body
    assert np.array_equal(child["sleep_device"].astype(bool), asleep)   # the device variant: the same


# ---- the closed loop --------------------------------------------------------------------------------------------------
def test_a_control_loop_that_stays_on_the_device_follows_the_model(child):
    rows, joints, lims, drvs = jc.loop_scene()
    drvs = drvs.copy()
    for _ in range(jc.LOOP_FRAMES):                                     # the same loop through the CPU models
        angle = jsm.joint_states(rows, joints, lims, drvs)[0][0]["angle"]
        drvs["target"][0] = jc.LOOP_GAIN * (jc.LOOP_GOAL - angle)
        rows = jd.step(rows, joints, lims, drvs, jc.DT, jc.SUBSTEPS)
    model_angle = jsm.joint_states(rows, joints, lims, drvs)[0][0]["angle"]
    device_angle = child["loop_state"][0]["angle"]
    model_error, device_error = abs(model_angle - jc.LOOP_GOAL), abs(device_angle - jc.LOOP_GOAL)
    print("closed loop: |angle - goal| model %.6g, device %.6g (asserted: %.6g); largest |device - model| over the rows %.3g"
          % (model_error, device_error, 4 * model_error, np.abs(child["loop_rows"] - rows).max()))
    np.testing.assert_allclose(child["loop_rows"], rows, rtol=0, atol=1e-10)
    assert model_error < 1e-4 * jc.LOOP_GOAL                            # the loop did converge (the wheel started at angle 0)
    assert device_error <= 4 * model_error
