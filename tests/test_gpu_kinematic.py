"""Kinematic bodies on the GPU (include/xpbd.h, "KINEMATIC bodies"): scripted poses and velocities that push and carry.

Expected frames are the committed oracle's, run one substep at a time with the model's velocities (tests/kinematic_model.py)
written into the kinematic bodies before each call; tests/test_kinematic_model.py shows that yardstick valid on these scenes.
Where a frame only translates no transcendental enters and every body must equal the expected frame bit for bit; positions and
linear velocities are the model's bits always.  Rotations and angular velocities go through the device's atan2 / tan, which
are not correctly rounded, and are held to a MEASURED tolerance.

TOLERANCE.  The largest deviation from the model over the arrival cases (65 bodies, S in {1, 3, 20}) was measured on an MI355X
(printed by the test; the figures are in DESIGN.md 8, "Kinematic bodies"): rotation components MEASURED_ROTATION, angular
velocity times h / 2 (the vector part of the rotation a substep made) MEASURED_ANGULAR.  The tests assert 20 times that: the
margin covers other inputs.

What cannot be seen from outside: the velocities between the substeps of one step.  What a frame leaves are derive's velocities
of its LAST substep, which follow from the r = 1 overwrite; the earlier overwrites show in the carried bodies (bit for bit
against the expected frames) and in the pose a frame of several substeps reaches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kinematic_common as kc
import kinematic_model as km
import oracle_binding as ob
import terrain_model as tm
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED_ROTATION = 3.331e-16  # largest |device - model| of a rotation component on the MI355X
MEASURED_ANGULAR = 3.158e-16   # largest |device - model| of an angular velocity component, times h / 2
ROTATION_TOLERANCE, ANGULAR_TOLERANCE = 20 * MEASURED_ROTATION, 20 * MEASURED_ANGULAR


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """kinematic_device_child.py, once: the device variant driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("kinematic") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "kinematic_device_child.py"), str(out)], capture_output=True, text=True, timeout=600)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):       # killed: nothing more is started on that GPU
        pytest.exit("kinematic_device_child.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["runs"] == 5
    return dict(np.load(out))


# ---- 1. carry -------------------------------------------------------------------------------------------------------------
def test_a_box_is_carried_by_a_translating_slab_bit_for_bit():
    bodies, sid = kc.carry_scene()
    want = kc.carry_expected()
    with kc.new_world(bodies, sid) as w:
        got = kc.run(w, kc.carry_tables(), kc.CARRY_SUBSTEPS)
        assert w.kinematic_count() == 1
    for f in range(kc.CARRY_FRAMES):
        assert bits_equal(got[f], want[f]), f
    assert got[-1][1, 31] > 0.5 * got[-1][0, 31] > 0.0                 # it was carried


# ---- 2. arrival -----------------------------------------------------------------------------------------------------------
def arrival_run(substeps):
    bodies, sid, tbl = kc.arrival_scene()
    with kc.new_world(bodies, sid) as w:
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, substeps)
        return w.download(), bodies, tbl


@pytest.mark.parametrize("substeps", kc.ARRIVAL_SUBSTEPS)
def test_pose_targets_are_reached_in_the_last_substep(substeps):
    rows, bodies, tbl = arrival_run(substeps)
    rot, ang, exact = kc.arrival_deviation(rows, substeps)
    print("S = %d: rotation deviation %.3e, angular deviation %.3e, positions and linear velocities the model's bits: %s" % (substeps, rot, ang, exact))
    for i in range(kc.N_ARRIVAL):
        for c in range(3):
            bound = 4.0 * np.spacing(max(abs(bodies[i, 31 + c]), abs(tbl[i]["linear"][c])))
            assert abs(rows[i, 31 + c] - tbl[i]["linear"][c]) <= bound, (i, c)
    assert exact                                                        # no transcendental enters the positions
    assert rot <= ROTATION_TOLERANCE and ang <= ANGULAR_TOLERANCE, (rot, ang)
    want = kc.arrival_model(substeps)
    spin_got, spin_want = np.linalg.norm(rows[kc.SPINNER, 25:28]), np.linalg.norm(want[kc.SPINNER, 10:13])
    h = kc.DT / substeps
    assert spin_want > 1.0 and abs(spin_got - spin_want) * h / 2.0 <= ANGULAR_TOLERANCE      # the spinner's speed is the model's


def test_the_set_dynamics_substitute_decays_and_never_arrives():
    """A fixed body given the spinner's first angular velocity through set_dynamics: after the frame it has lost speed and has
    not reached the orientation (what the kinematic entry is for)."""
    bodies, sid, tbl = kc.arrival_scene()
    substeps = 20
    h = kc.DT / substeps
    _, w0 = km.pose_velocities(tuple(bodies[kc.SPINNER, 31:34]), tuple(bodies[kc.SPINNER, 34:38]), tuple(tbl[kc.SPINNER]["linear"]),
                               tuple(tbl[kc.SPINNER]["angular"]), h, substeps)
    with kc.new_world(bodies, sid) as w:
        row = w.get_dynamics([kc.SPINNER])
        row[0, 10:13] = w0
        w.set_dynamics([kc.SPINNER], row)
        w.step(kc.DT, substeps)
        got = w.download()[kc.SPINNER]
    speed0, speed = float(np.linalg.norm(w0)), float(np.linalg.norm(got[25:28]))
    per_substep = (2.0 / h) * np.sin(np.arctan(h * speed0 / 2.0)) / speed0
    print("substitute: %.6f of the speed left after %d substeps (model %.6f)" % (speed / speed0, substeps, per_substep ** substeps))
    assert speed < speed0 * (1.0 - 0.5 * (1.0 - per_substep ** substeps))
    assert np.abs(got[34:38] - tbl[kc.SPINNER]["angular"]).max() > 100 * max(ROTATION_TOLERANCE, 1e-12)


# ---- 3. VELOCITY mode -----------------------------------------------------------------------------------------------------
def test_velocity_mode_moves_carries_and_stops():
    bodies, sid, tbl = kc.velocity_scene()
    tables = [tbl] * kc.VELOCITY_FRAMES
    want = kc.expected(bodies, sid, tables, kc.VELOCITY_SUBSTEPS)
    with kc.new_world(bodies, sid) as w:
        got = kc.run(w, tables, kc.VELOCITY_SUBSTEPS)
        for f in range(kc.VELOCITY_FRAMES):
            for i in (kc.CONVEYOR, kc.RIDER):                           # angular == 0: bit for bit
                assert bits_equal(got[f][i], want[f][i]), (f, i)
            # a VELOCITY entry's angular velocity is copied, not computed: no transcendental enters here either, and on the
            # MI355X the spinning bodies were the expected bits too (measured deviation 0); they are held to the measured tolerance
            # of the POSE cases all the same, their positions and linear velocities to the bit
            for i in (kc.TURNTABLE, kc.BOTH):
                assert bits_equal(got[f][i, 31:34], want[f][i, 31:34]) and bits_equal(got[f][i, 22:25], want[f][i, 22:25]), (f, i)
                rot = np.abs(got[f][i, 34:38] - want[f][i, 34:38]).max()
                ang = np.abs(got[f][i, 25:28] - want[f][i, 25:28]).max() * (kc.DT / kc.VELOCITY_SUBSTEPS) / 2.0
                print("frame %d body %d: rotation deviation %.3e, angular deviation %.3e" % (f, i, rot, ang))
                assert rot <= ROTATION_TOLERANCE and ang <= ANGULAR_TOLERANCE, (f, i, rot, ang)
        assert got[-1][kc.CONVEYOR, 31] > bodies[kc.CONVEYOR, 31] + 0.01 and got[-1][kc.RIDER, 31] > bodies[kc.RIDER, 31]
        speed = np.linalg.norm(got[-1][kc.TURNTABLE, 25:28]) / np.linalg.norm(tbl[kc.TURNTABLE]["angular"][:3])
        assert abs(speed - 1.0) < 1e-3 and speed > 0.9999                # re-asserted every substep: what is left is one substep's loss
        # the conveyor's entry to zero velocity: it stands still, bit-frozen
        w.set_kinematic_targets([kc.CONVEYOR], np.zeros((1, 7)))
        w.step(kc.DT, kc.VELOCITY_SUBSTEPS)
        still = w.download()[kc.CONVEYOR]
        assert bits_equal(still[31:38], got[-1][kc.CONVEYOR, 31:38]) and not still[22:28].any()
        w.step(kc.DT, kc.VELOCITY_SUBSTEPS)
        assert bits_equal(w.download()[kc.CONVEYOR], still)


# ---- 4. retarget ----------------------------------------------------------------------------------------------------------
def test_host_retarget_equals_the_whole_table_with_the_new_rows():
    for entries, rows in ((None, kc.new_rows()), kc.some_entries()):
        got = kc.retarget_run(kc.host_retarget, entries, rows)
        assert bits_equal(got, kc.retarget_run(kc.table_retarget, entries, rows))
        assert not bits_equal(got, kc.retarget_run(lambda *a: None, entries, rows))     # it matters


def test_device_retarget_equals_the_host_retarget(child):
    assert bits_equal(child["all"], kc.retarget_run(kc.host_retarget, None, kc.new_rows()))
    assert bits_equal(child["some"], kc.retarget_run(kc.host_retarget, *kc.some_entries()))


def test_invalid_entries_are_skipped_on_the_device_and_refused_by_the_host(child):
    entries, rows, valid = kc.invalid_list()
    assert bits_equal(child["invalid"], kc.retarget_run(kc.table_retarget, entries[valid], rows[valid]))
    refused = []

    def host(w, tbl, e, r):
        with pytest.raises(capi.XpbdError) as err:
            w.set_kinematic_targets(e, r)
        refused.append(err.value.code)

    untouched = kc.retarget_run(host, entries, rows)
    assert refused == [capi.E_INVALID]
    assert bits_equal(untouched, kc.retarget_run(lambda *a: None, None, None))


def test_rows_set_on_the_device_survive_a_population_change(child):
    assert bits_equal(child["remove_kept"], child["remove_fresh"])


# ---- 5. empty table -------------------------------------------------------------------------------------------------------
def test_a_cleared_table_steps_like_a_world_that_never_had_one():
    bodies, sid = kc.stacks_scene()

    def frames(touch):
        with kc.new_world(bodies, sid) as w:
            if touch:
                w.set_kinematics(kc.to_capi(kc.slab_tables(0.01, 1)[0]))
                assert w.kinematic_count() == 2
                w.set_kinematics(None)
                assert w.kinematic_count() == 0
            out = []
            for _ in range(3):
                w.step(kc.DT, 4)
                out.append(w.download())
            return out

    plain = frames(False)
    assert all(bits_equal(a, b) for a, b in zip(frames(True), plain))
    want = bodies
    for f in range(3):                                                 # ... which is the oracle's frame: the fused schedule's result
        want = ob.contacts_step_joints(want, sid, kc.polys(), kc.NO_JOINTS, kc.DT, 4, kc.PAD)
        assert bits_equal(plain[f], want), f


def test_refusals_leave_the_table_as_it_was_and_the_split_api_is_closed():
    bodies, sid = kc.stacks_scene()
    tbl = kc.slab_tables(0.01, 1)[0]
    with kc.new_world(bodies, sid) as w:
        w.set_kinematics(kc.to_capi(tbl))
        bad = tbl.copy()
        bad["body"][1] = 5                                              # a body with mass
        with pytest.raises(capi.XpbdError) as err:
            w.set_kinematics(kc.to_capi(bad))
        assert err.value.code == capi.E_INVALID and "not fixed" in str(err.value)
        assert w.kinematic_count() == 2
        for call in (lambda: hip_call(w, "xpbd_world_contacts_begin", kc.DT), lambda: hip_call(w, "xpbd_world_contacts_substep", kc.DT)):
            assert call() == capi.E_INVALID
        w.step(kc.DT, 4)                                                # the old table is in force: slab A travels
        assert abs(w.download()[kc.SLAB_A, 33] - 2.01) <= 4.0 * np.spacing(2.01)
        w.upload(bodies, sid)                                           # an upload clears it, as it clears joints
        assert w.kinematic_count() == 0


def hip_call(w, name, value):
    import ctypes as C
    fn = getattr(capi.hip_lib(), name)
    fn.argtypes = [C.c_void_p, C.c_double]
    return fn(w._h, value)


# ---- 7. combinations ------------------------------------------------------------------------------------------------------
def model_frame(model, tbl, substeps):
    """One frame of a material / restitution / terrain model with the table's overwrite where the step has it: before the
    broadphase for the first substep, before the integrate stage for the others."""
    h = kc.DT / substeps
    model.bodies[:], _ = km.overwrite(model.bodies, tbl, h, substeps)
    off, nb = ob.broadphase(model.bodies, model.sid, model.polys, kc.DT, model.pad)
    for k in range(substeps):
        if k:
            model.bodies[:], _ = km.overwrite(model.bodies, tbl, h, substeps - k)
        model.substep(off, nb, h)
    return model.bodies.copy()


def lift_scene():
    """A kinematic slab (body 0) rising 5 cm per frame under a resting box (1); a free box resting on the ground 10 m away (2)."""
    bodies, sid = kc.boxes(3, [[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [10.0, 0.0, 0.0]], fixed=[0])
    return bodies, sid, km.table((0, km.POSE, [0.02, 0.0, 1.05], kc.IDENT))


def test_one_frame_with_restitution_is_the_models_bits():
    bodies, sid, tbl = lift_scene()
    e = [0.5, 0.5, 0.5]
    model = tm.Model(bodies, sid, kc.polys(), None, e=e, ground_e=0.5, pad=kc.PAD)
    want = model_frame(model, tbl, 8)
    assert model.pair_entries >= 1                                      # the slab's push bounced the box: the pass had work
    with kc.new_world(bodies, sid) as w:
        w.set_restitution(e, 0.5, 0.0)
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, 8)
        assert bits_equal(w.download(), want)


def test_one_frame_on_a_terrain_is_the_models_bits():
    bodies, sid, tbl = lift_scene()
    bodies[2, 33] = 0.3
    origin, cell = (-4.0, -4.0), (8.0, 8.0)
    heights = tm.tilted_field(4, 3, origin, cell, 0.05, 0.02)
    model = tm.Model(bodies, sid, kc.polys(), tm.Terrain(heights, origin, cell), pad=kc.PAD)
    want = model_frame(model, tbl, 8)
    with kc.new_world(bodies, sid) as w:
        w.set_terrain(heights, origin, cell)
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, 8)
        got = w.download()
    assert bits_equal(got, want) and not np.isnan(want).any()
    assert want[1, 33] > bodies[1, 33] + 0.01                           # the box went up with the slab


def hanging_scene():
    """A kinematic anchor (body 0) translating sideways, a box (1) hanging from it by a distance joint, one (2) hinged to it."""
    bodies, sid = kc.boxes(3, [[0.0, 0.0, 8.0], [0.0, 0.0, 6.0], [2.0, 0.0, 8.0]], fixed=[0])
    joints = np.zeros(2, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = [0, 0], [1, 2]
    joints["anchor_a"], joints["anchor_b"] = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]], [[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5]]
    joints["distance"] = [2.0, 0.0]
    joints["axis_a"][1] = joints["axis_b"][1] = [0.0, 1.0, 0.0]
    joints["kind"] = [capi.JOINT_DISTANCE, capi.JOINT_HINGE]
    return bodies, sid, joints, km.table((0, km.POSE, [0.04, -0.02, 8.03], kc.IDENT))


def test_one_frame_with_joints_anchored_to_a_kinematic_body_is_the_oracles_bits():
    bodies, sid, joints, tbl = hanging_scene()
    want = kc.expected(bodies, sid, [tbl], 10, joints)[0]
    with kc.new_world(bodies, sid, joints) as w:
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, 10)
        got = w.download()
    assert bits_equal(got, want)
    assert np.abs(want[1:, 31:34] - bodies[1:, 31:34]).max() > 1e-3     # the anchor dragged both along


def test_a_drive_anchored_to_a_kinematic_body_equals_its_twin_stepped_substep_by_substep():
    """No reference in the suite gives a driven joint's bits (the drive model is held to 1e-10), so the yardstick here is the
    library itself: a twin without a table, stepped one substep per call, with the model's velocities written into the anchor
    through set_dynamics before each call.  With the anchor static, the twin per substep equals the world per frame (first)."""
    bodies, sid, joints, tbl = hanging_scene()
    x = [1.0, 0.0, 0.0]
    drive = np.zeros(1, dtype=capi.JOINT_DRIVE_DTYPE)
    drive["joint"], drive["kind"], drive["ref_a"], drive["ref_b"] = 1, capi.DRIVE_ANGULAR_VELOCITY, x, x
    drive["target"], drive["compliance"], drive["max_force"] = 1.5, 0.0, np.inf
    substeps, h = 10, kc.DT / 10

    def world():
        w = kc.new_world(bodies, sid, joints)
        w.set_joint_drives(drive)
        return w

    def twin(table):
        with world() as t:
            for k in range(substeps):
                if table is not None:
                    rows, _ = km.overwrite(t.download(), table, h, substeps - k)
                    dyn = t.get_dynamics([0])
                    dyn[0, 7:13] = rows[0, 22:28]
                    t.set_dynamics([0], dyn)
                t.step(h, 1)
            return t.download()

    with world() as w:
        w.step(kc.DT, substeps)
        assert bits_equal(w.download(), twin(None))                     # the yardstick, anchor static
    with world() as w:
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, substeps)
        got = w.download()
    assert bits_equal(got, twin(tbl))
    assert abs(got[2, 26]) > 0.01                                       # the hinged box turns about the hinge


# ---- 8. population and history --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gone", [0, 4], ids=["below_a_kinematic_body", "a_kinematic_body"])
def test_after_a_removal_the_world_steps_like_a_fresh_one_with_the_reindexed_table(gone):
    bodies, sid, tbl = kc.retarget_scene()
    tbl = tbl[tbl["body"] >= 2]                                         # bodies 0 and 1 stay plain fixed bodies
    with kc.new_world(bodies, sid) as w:
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, kc.RETARGET_SUBSTEPS)
        old_to_new, _ = w.remove_bodies([gone])
        kept = tbl[tbl["body"] != gone].copy()
        kept["body"] = old_to_new[kept["body"]]
        assert w.kinematic_count() == len(kept) == len(tbl) - (1 if gone >= 2 else 0)
        at_change = w.download()
        for _ in range(kc.RETARGET_THEN):
            w.step(kc.DT, kc.RETARGET_SUBSTEPS)
        got = w.download()
    with kc.new_world(at_change, np.delete(sid, gone)) as f:
        f.set_kinematics(kc.to_capi(kept))
        for _ in range(kc.RETARGET_THEN):
            f.step(kc.DT, kc.RETARGET_SUBSTEPS)
        assert bits_equal(got, f.download())
    assert np.abs(got[:, 31:34] - at_change[:, 31:34]).max() > 1e-3     # the VELOCITY entries kept moving their bodies


def test_history_restore_then_the_same_targets_reproduces_the_run():
    bodies, sid, tbl = kc.retarget_scene()
    later = [kc.new_rows(3), kc.new_rows(4)]
    with kc.new_world(bodies, sid) as w:
        w.set_kinematics(kc.to_capi(tbl))
        w.step(kc.DT, kc.RETARGET_SUBSTEPS)
        index = w.history_push()

        def rest():
            out = []
            for rows in later:
                w.set_kinematic_targets(None, rows)
                w.step(kc.DT, kc.RETARGET_SUBSTEPS)
                out.append(w.download())
            return out

        first = rest()
        w.history_restore(index)
        assert w.kinematic_count() == len(tbl)                          # the table is not part of an entry: the last rows stand
        again = rest()
    assert all(bits_equal(a, b) for a, b in zip(first, again)) and not bits_equal(first[0], first[1])
