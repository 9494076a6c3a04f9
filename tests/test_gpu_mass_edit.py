"""Mass edits on the GPU (include/xpbd.h, "MASS properties of resident bodies"): freeze, release, re-weigh.

The property everything rests on is held bit for bit: a world after the call steps like a fresh world into which the download
taken after the call was uploaded, with the same settings set again -- bodies, per-substep contact masks and the contact report.
The block scenes start on the contact pipeline's shared per-shape mass table and leave it with the edit; the all-bodies variant
ends with a fresh world that shares again and an edited one that does not.  What an edit writes is the model's bits
(tests/mass_edit_model.py, itself held to the oracle and to rational arithmetic by tests/test_mass_edit_model.py).

KEEP_FRAME BOUND.  The frame after the edit differs from the frame before it by at most 64 * 2^-53 * M per component, M the
largest absolute component of the body's position, old and new centre of mass: the two formulas round position' once at
magnitude <= M + 6|d| and each of the two frame evaluations rounds twice at magnitude <= 2M, the rotated terms are below |com|
and carry a few roundings of their own.  Measured on an MI355X over the 16 bodies: 1.42 * 2^-53 * M (printed by the test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import islands_common as ic
import mass_edit_common as mc
import mass_edit_model as mm
from constraint_solver_amd import capi
from mass_edit_common import same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
N_CHILD_RUNS = 17


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """mass_edit_device_child.py, once: the device variant driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("mass_edit") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "mass_edit_device_child.py"), str(out)], capture_output=True, text=True, timeout=600)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):       # killed: nothing more is started on that GPU
        pytest.exit("mass_edit_device_child.py died with status %d:\n%s" % (p.returncode, p.stderr[-3000:]), returncode=1)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["runs"] == N_CHILD_RUNS
    return dict(np.load(out))


def refused(call, code=capi.E_INVALID):
    with pytest.raises(capi.XpbdError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


# ---- 1. get / set round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(mc.TRIP_LISTS))
def test_get_is_the_columns_of_download_and_set_writes_the_rows_and_nothing_else(which, child):
    before, got_before, after, got_after, rows = mc.trip_run(mc.host_edit, which)
    idx = np.arange(mc.N_TRIP) if mc.TRIP_LISTS[which] is None else np.array(mc.TRIP_LISTS[which])
    assert same(got_before, before[idx][:, mc.MASS])
    assert same(after[idx][:, mc.MASS], rows) and same(got_after, rows)
    assert same(after[:, mc.OTHERS], before[:, mc.OTHERS])                # the other 25 doubles of every body: the same bits
    rest = np.setdiff1d(np.arange(mc.N_TRIP), idx)
    assert same(after[rest], before[rest])
    assert same(after, mm.apply(before, idx, rows, mm.INVERSE)[0])
    assert same(child["trip_" + which], after) and same(child["trip_get_" + which], rows)        # the device variant: the same bits


# ---- 2. the property, from the shared-mass path ----------------------------------------------------------------------------
def assert_block_steps_like_a_fresh_world(edits_of, narrowphase):
    edited, got = mc.block_run(mc.host_edit, edits_of, narrowphase)
    want = mc.block_fresh(edited, narrowphase)
    # (the first frame's events are reported against S_prev, which a fresh world does not have; everything else must agree)
    for k in range(mc.POST_FRAMES):
        for name in ("bodies", "contacts", "masks", "pairs", "points") + (("events", "counts") if k else ()):
            a, b = getattr(got[k], name), getattr(want[k], name)
            assert (a == b if isinstance(a, tuple) else same(a, b)), (k, name)
    assert len(got[-1].pairs) > 0 and got[-1].masks.any()              # the block has landed: pairs and ground contacts
    return edited, got


@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA], ids=["sat", "gjk_epa"])
def test_three_edited_bodies_step_like_a_fresh_world_with_the_same_settings(narrowphase):
    edited, got = assert_block_steps_like_a_fresh_world(mc.block_edits, narrowphase)
    bodies, _ = mc.block_scene()
    assert same(edited[mc.HEAVY, 0:10], bodies[mc.HEAVY, 0:10] / 10.0) and not edited[mc.FROZEN, 0:10].any()
    assert edited[mc.SHIFTED, 28] == bodies[mc.SHIFTED, 28] + 0.1
    last = got[-1].bodies
    # the edit matters: the unedited block ends elsewhere
    _, plain = mc.block_run(mc.host_edit, lambda rows: [])
    assert not same(plain[-1].bodies[:, mc.DYN], last[:, mc.DYN])


def test_all_bodies_edited_to_one_row_step_like_a_fresh_world_that_shares_again():
    edited, _ = assert_block_steps_like_a_fresh_world(mc.all_edit, capi.NARROWPHASE_SAT)
    assert len(np.unique(edited[:, mc.MASS], axis=0)) == 1


@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP], ids=["fused", "per_substep"])
def test_the_property_holds_in_the_ground_only_modes(mode):
    bodies, sid = mc.boxes([[3.0 * i, 0.0, 0.01 + 0.1 * i] for i in range(8)])
    bodies[:, 25:28] = [0.3, -0.2, 0.1]
    with mc.new_world(bodies, sid, mode=mode) as a:
        for _ in range(mc.PRE_FRAMES):
            a.step(mc.DT, mc.SUBSTEPS)
        rows = a.get_mass_properties()
        heavy, frozen, shifted = rows[1].copy(), rows[4].copy(), rows[6].copy()
        heavy[0:10] /= 10.0
        frozen[0:10] = 0.0
        shifted[10] += 0.1
        a.set_mass_properties([4, 1], np.stack([frozen, heavy]))
        a.set_mass_properties([6], shifted, mm.INVERSE | mm.KEEP_FRAME)
        edited = a.download()
        for _ in range(mc.POST_FRAMES):
            a.step(mc.DT, mc.SUBSTEPS)
        got = (a.download(), a.contacts())
    with mc.new_world(edited, sid, mode=mode) as b:
        for _ in range(mc.POST_FRAMES):
            b.step(mc.DT, mc.SUBSTEPS)
        want = (b.download(), b.contacts())
    assert same(got[0], want[0]) and same(got[1], want[1]) and len(got[1])


# ---- 3. DIRECT -------------------------------------------------------------------------------------------------------------------
def test_direct_rows_are_inverted_to_the_models_bits(child):
    idx, rows = mc.direct_rows()
    before, after = mc.direct_run(mc.host_edit)
    want, verdicts = mm.apply(before, idx, rows, mm.DIRECT)
    assert verdicts == [mm.OK] * mc.N_DIRECT
    assert same(after, want) and not same(after[idx][:, 0:10], before[idx][:, 0:10])
    assert same(child["direct"], after)


def test_a_singular_row_is_refused_by_the_host_and_skipped_alone_on_the_device(child):
    idx, rows = mc.direct_rows(singular=True)
    bodies, sid = mc.direct_scene()
    with mc.new_world(bodies, sid) as w:
        before = w.download()
        message = refused(lambda: w.set_mass_properties(idx, rows, mm.DIRECT), capi.E_SINGULAR_INERTIA)
        assert "xpbd_world_set_mass_properties" in message and "rows[%d]" % mc.SINGULAR_AT in message
        assert same(w.download(), before)
    want, verdicts = mm.apply(before, idx, rows, mm.DIRECT)
    assert verdicts.count(mm.SINGULAR) == 1 and verdicts[mc.SINGULAR_AT] == mm.SINGULAR
    assert same(child["direct_singular_before"], before) and same(child["direct_singular"], want)
    assert same(want[idx[mc.SINGULAR_AT]], before[idx[mc.SINGULAR_AT]])


# ---- 4. KEEP_FRAME -----------------------------------------------------------------------------------------------------------
def test_keep_frame_moves_position_and_velocity_to_the_models_bits_and_the_frame_stays(child):
    before, frames_before, after, frames_after, rows = mc.keep_run(mc.host_edit)
    want, _ = mm.apply(before, None, rows, mm.INVERSE | mm.KEEP_FRAME)
    assert same(after, want)
    assert same(after[:, 34:38], before[:, 34:38]) and same(after[:, 25:28], before[:, 25:28])           # rotation, angular velocity
    assert not same(after[:, 31:34], before[:, 31:34]) and not same(after[:, 22:25], before[:, 22:25])
    model_frames = np.array([list(mm.frame_origin(tuple(b[31:34]), tuple(b[34:38]), tuple(b[28:31]))) + list(b[34:38]) for b in want])
    assert same(frames_after, model_frames)
    worst = 0.0
    for i in range(mc.N_KEEP):
        m = max(np.abs(before[i, 31:34]).max(), np.abs(before[i, 28:31]).max(), np.abs(rows[i, 10:13]).max())
        moved = np.abs(frames_after[i, 0:3] - frames_before[i, 0:3]).max()
        worst = max(worst, moved / (U * m))
        assert moved <= 64 * U * m, (i, moved / (U * m))
    print("KEEP_FRAME: the frame moved by at most %.2f * 2^-53 * M (bound 64)" % worst)
    assert same(frames_after[:, 3:7], frames_before[:, 3:7])
    assert same(child["keep"], after) and same(child["keep_frames"], frames_after)


# ---- 5. freeze and release ------------------------------------------------------------------------------------------------------
def test_a_frozen_box_keeps_its_bits_under_a_falling_one_and_release_restores_the_mass():
    """The lower box is uploaded at rest on the plane and frozen before the first step: a fixed body moves at whatever velocity
    it has (see "KINEMATIC bodies"), so only a body that is exactly at rest stays where it is; a host that freezes a moving
    body also stops it with xpbd_world_set_dynamics."""
    bodies, sid = mc.boxes([[0.0, 0.0, 0.0], [0.1, 0.05, 1.05]])
    with mc.new_world(bodies, sid) as w:
        saved = w.get_mass_properties([0])
        assert same(saved, bodies[[0]][:, mc.MASS])
        zeros = saved.copy()
        zeros[0, 0:10] = 0.0
        w.set_mass_properties([0], zeros)
        frozen = w.download()
        assert same(frozen[:, mc.OTHERS], bodies[:, mc.OTHERS])
        landed = False
        for _ in range(10):
            w.step(mc.DT, mc.SUBSTEPS)
            now = w.download()
            assert same(now[0, mc.DYN], frozen[0, mc.DYN])                # all 13 dynamic doubles keep their bits
            landed = landed or abs(now[1, 33] - 1.0) < 0.02
        assert landed                                                    # the other box came to lie on it
        w.set_mass_properties([0], saved)
        assert same(w.get_mass_properties([0]), saved)
        released = w.download()
        assert same(released[0, mc.MASS], bodies[0, mc.MASS]) and same(released[:, mc.OTHERS], now[:, mc.OTHERS])
        for _ in range(3):
            w.step(mc.DT, mc.SUBSTEPS)
        got = w.download()
    with mc.new_world(released, sid) as f:
        for _ in range(3):
            f.step(mc.DT, mc.SUBSTEPS)
        assert same(got, f.download())


# ---- 6. grab, carry, release ----------------------------------------------------------------------------------------------------
def test_grab_carry_release(child):
    bodies, sid = mc.boxes([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0]])
    with mc.new_world(bodies, sid) as w:
        for _ in range(3):
            w.step(mc.DT, mc.SUBSTEPS)
        saved = w.get_mass_properties([0])
        zeros = saved.copy()
        zeros[0, 0:10] = 0.0
        refused(lambda: w.set_kinematics(capi.kinematics([0], capi.KINEMATIC_POSE, [[0.0, 0.0, 0.5]], [mc.IDENT])))     # it still has mass
        w.set_mass_properties([0], zeros)                                # freeze
        at = w.download()[0, 31:34]
        target = at + [0.0, 0.0, 0.5]
        w.set_kinematics(capi.kinematics([0], capi.KINEMATIC_POSE, [target], [mc.IDENT]))
        w.step(mc.DT, mc.SUBSTEPS)
        carried = w.download()
        assert same(carried[0, 31:34], target)                            # it arrives exactly
        w.step(mc.DT, mc.SUBSTEPS)                                        # the target persists: it holds, and its travel velocity is gone
        carried = w.download()
        assert same(carried[0, 31:34], target) and np.abs(carried[0, 22:28]).max() < 1e-12
        # mass while the entry exists: refused, nothing changes -- also for the other, legal entry of the same call
        both = np.concatenate([saved, w.get_mass_properties([1])])
        both[1, 0:10] /= 2.0
        message = refused(lambda: w.set_mass_properties([0, 1], both))
        assert "kinematic table" in message and same(w.download(), carried)
        zeros_moved = zeros.copy()
        zeros_moved[0, 10:13] += 0.05
        w.set_mass_properties([0], zeros_moved)                          # a row that leaves it fixed is taken
        w.set_mass_properties([0], zeros)
        w.set_kinematics(np.zeros(0, dtype=capi.KINEMATIC_DTYPE))                # clear the table
        w.set_mass_properties([0], saved)                                # release
        assert same(w.get_mass_properties([0]), saved)
        for _ in range(8):
            w.step(mc.DT, mc.SUBSTEPS)
        fell = w.download()
        assert fell[0, 33] < target[2] - 0.02 and fell[0, 24] < 0.0
    # the device variant skips the entry that breaks the rule and applies the legal entries of the same call
    want, verdicts = mm.apply(child["skip_before"], child["skip_idx"], child["skip_rows"], mm.INVERSE, kinematic={2, 3})
    assert verdicts == [mm.OK, mm.OK, mm.KINEMATIC_RULE, mm.OK, mm.OUT_OF_RANGE, mm.OUT_OF_RANGE, mm.NOT_FINITE, mm.NEGATIVE_INVERSE_MASS, mm.OK]
    assert same(child["skip_after"], want) and not same(want, child["skip_before"])


# ---- 10. a device edit and the step behind it on one stream ----------------------------------------------------------------------
def test_a_device_edit_followed_by_a_step_without_a_wait_equals_edit_wait_step(child):
    _, host = mc.block_run(mc.host_edit, mc.block_edits)
    assert same(child["no_wait"], child["waited"]) and same(child["waited"], host[-1].bodies)


# ---- 8. islands ------------------------------------------------------------------------------------------------------------------
def test_islands_see_a_frozen_body_as_an_anchor():
    """(Scene of 7(c) without sleeping: the middle box of a resting 3-stack is made fixed.)"""
    bodies, sid = mc.stacks_scene()
    joints = ic.distance_joints([], [])
    with mc.new_world(bodies, sid) as w:
        w.set_contact_report(True)
        for _ in range(5):
            w.step(mc.DT, mc.SUBSTEPS)
        of_before, before = ic.assert_equals_model(w, joints, 0)
        assert len({int(of_before[i]) for i in mc.STACK_A}) == 1        # one island
        zeros = w.get_mass_properties([mc.MIDDLE])
        zeros[0, 0:10] = 0.0
        w.set_mass_properties([mc.MIDDLE], zeros)
        of_now, now = ic.assert_equals_model(w, joints, 0)              # islands read the mass properties per call
        assert of_now[mc.MIDDLE] == capi.ISLAND_NONE
        lower, upper = of_now[mc.STACK_A[0]], of_now[mc.STACK_A[2]]
        assert lower != upper and capi.ISLAND_NONE not in (lower, upper)   # the 3-stack has split
        assert now["n_anchors"][lower] >= 1 and now["n_anchors"][upper] == 1 and len(now) == len(before) + 1
        w.step(mc.DT, mc.SUBSTEPS)
        ic.assert_equals_model(w, joints, 0)


# ---- 9. population and history -------------------------------------------------------------------------------------------------
def test_an_edited_row_survives_a_removal_and_a_history_restore():
    bodies, sid = mc.trip_scene()
    rows = mc.trip_rows(2, seed=6600)[::-1]
    with mc.new_world(bodies, sid) as w:
        w.step(mc.DT, mc.SUBSTEPS)
        assert w.history_push() == 0
        pushed = w.download()
        w.set_mass_properties([4, 2], rows, mm.INVERSE | mm.KEEP_FRAME)
        edited = w.download()
        assert not same(edited[[4, 2]][:, 31:34], pushed[[4, 2]][:, 31:34])          # KEEP_FRAME moved the positions ...
        w.step(mc.DT, mc.SUBSTEPS)
        w.history_restore(0)
        restored = w.download()
        assert same(restored[:, mc.DYN], pushed[:, mc.DYN])                          # ... the dynamic doubles come back
        assert same(restored[:, mc.MASS], edited[:, mc.MASS]) and same(w.get_mass_properties([4, 2]), rows)     # the edited mass stays
        old_to_new, _ = w.remove_bodies([3])
        assert same(w.get_mass_properties([old_to_new[4], old_to_new[2]]), rows)
        assert same(w.download(), np.delete(restored, 3, axis=0))


# ---- refusals through the library -------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_the_split_api_asks_for_a_new_broadphase():
    bodies, sid = mc.trip_scene()
    good = mc.trip_rows(2, seed=6700)
    with mc.new_world(bodies, sid) as w:
        w.step(mc.DT, mc.SUBSTEPS)
        before = w.download()
        nan, negative = good.copy(), good.copy()
        nan[1, 7], negative[0, 0] = np.nan, -1.0
        for call in (lambda: w.set_mass_properties([1, 7], good), lambda: w.set_mass_properties([1, 1], good),
                     lambda: w.set_mass_properties(None, good), lambda: w.set_mass_properties([1, 2], good, 2),
                     lambda: w.set_mass_properties([1, 2], good, 0x200), lambda: w.set_mass_properties([1, 2], nan),
                     lambda: w.set_mass_properties([1, 2], negative), lambda: w.set_mass_properties([1, 2], negative, mm.DIRECT),
                     lambda: w.get_mass_properties([7]), lambda: w.set_mass_properties_device(0, 2, 0, 0),
                     lambda: w.set_mass_properties_device(0, 2, 8, 0), lambda: w.set_mass_properties_device(0, mc.N_TRIP, 12, 0),
                     lambda: w.set_mass_properties_device(0, mc.N_TRIP, 8, 0x202)):
            assert "xpbd_world_" in refused(call)
        assert same(w.download(), before)
        w.set_mass_properties([], np.zeros((0, 13)))                      # n == 0 does nothing
        assert same(w.download(), before)
        w.contacts_begin(mc.DT)
        w.contacts_substep(mc.DT / 4)
        w.set_mass_properties([1, 2], good)
        assert "contacts_begin" in refused(lambda: w.contacts_substep(mc.DT / 4))
        w.contacts_begin(mc.DT)
        w.contacts_substep(mc.DT / 4)
