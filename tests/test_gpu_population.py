"""Body population (include/xpbd.h, "Body POPULATION") on the GPU: removing resident bodies and appending new ones without an
upload.  The property everything rests on -- a world after a population change steps bit for bit like a fresh world given
its download and the settings re-indexed by the test itself (numpy, from old_to_new) -- in every mode and under both
narrowphases; the download right after the change; the maps against np.cumsum at every scan boundary; the device variant
from a torch stream; joints with limits and drives; settings that are off stay off; rejected calls change nothing; and 20
rounds of churn against a twin driven through download / upload / re-set.  EXTENSION: parity unpinned."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import body_edit_common as bc
import population_common as pc
from body_edit_common import DT, N, STATIC_BODY, SUBSTEPS, scene, world
from constraint_solver_amd import capi
from halo_common import pile
from population_common import NO_HIT, REMOVED, apply_settings, expected_map, newcomers, reindex_joints, reindex_settings, same_runs, settings_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MIXED, BOXES = capi.SCENE_MIXED_DROP, capi.SCENE_BOXES_DROP
MODES = [(capi.MODE_FUSED, capi.NARROWPHASE_SAT), (capi.MODE_PER_SUBSTEP, capi.NARROWPHASE_SAT),
         (capi.MODE_CONTACTS, capi.NARROWPHASE_SAT), (capi.MODE_CONTACTS, capi.NARROWPHASE_GJK_EPA)]
N_ADD = 4


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the property everything rests on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [MIXED, BOXES])
@pytest.mark.parametrize("mode,narrowphase", MODES)
def test_a_changed_world_steps_like_a_fresh_world_with_reindexed_settings(kind, mode, narrowphase):
    contacts_mode = mode == capi.MODE_CONTACTS                           # (joints, and so the full settings, need the contact pipeline)
    bodies, sid = scene(kind)
    s = settings_for()
    fresh, fresh_sid = newcomers(kind, N_ADD)
    force, torque = bc.wrench_values(3)
    want_map, keep = expected_map(N, REMOVED)
    with world(kind, bodies, sid, mode, narrowphase) as a:
        if contacts_mode:
            apply_settings(a, s)
        a.set_external_wrench(None, force, torque)
        a.step(DT, SUBSTEPS)
        before = a.download()
        old_to_new, joint_map = a.remove_bodies(REMOVED)
        assert a.add_bodies(fresh, fresh_sid) == N - 5
        assert a.n == N - 5 + N_ADD
        changed = a.download()
        got = pc.run(a, 3, contacts_mode)
    assert same(old_to_new, want_map)
    assert same(changed, np.concatenate([before[keep], fresh]))
    changed_sid = np.concatenate([sid[keep], fresh_sid])
    with world(kind, changed, changed_sid, mode, narrowphase) as b:
        if contacts_mode:
            r = reindex_settings(s, want_map, N_ADD)
            assert same(joint_map, reindex_joints(s, want_map)[3]) and len(r["joints"]) < len(s["joints"])
            apply_settings(b, r)
        want = pc.run(b, 3, contacts_mode)
    assert same_runs(got, want)
    if contacts_mode:
        assert len(got[0]) and len(got[2])                              # pairs were reported, and events (all BEGINs: S_prev is gone)
        assert (got[2]["kind"] == capi.CONTACT_BEGIN).all()
    with world(kind, bodies, sid, mode, narrowphase) as c:               # ... and the change matters to the run
        if contacts_mode:
            apply_settings(c, s)
        c.set_external_wrench(None, force, torque)
        c.step(DT, SUBSTEPS)
        unchanged = pc.run(c, 3, contacts_mode)
    at = -4 if contacts_mode else -2
    # in the contact pipeline the survivors miss the removed bodies (contacts, joints) and meet the new ones; in the ground-only
    # modes bodies do not interact, so the survivors must not notice the change at all
    assert same(unchanged[at][keep], got[at][:N - 5]) == (not contacts_mode)


# ---- 2. the download right after the change ------------------------------------------------------------------------------------
def test_download_after_the_change_is_the_kept_rows_then_the_added_rows():
    bodies, sid = scene(MIXED)
    force, torque = bc.wrench_values(5)
    fresh, fresh_sid = newcomers(MIXED, N_ADD)
    _, keep = expected_map(N, REMOVED)
    with world(MIXED, bodies, sid) as w:
        listed = np.array([4, 6, 62, 65, 128, STATIC_BODY], dtype=np.uint32)       # neighbours of removed bodies among them
        w.set_external_wrench(listed, force[listed], torque[listed])
        w.step(DT, SUBSTEPS)
        before = w.download()
        w.remove_bodies(REMOVED)
        after_remove = w.download()
        first = w.add_bodies(fresh, fresh_sid)
        after_add = w.download()
    assert same(before[listed][:, 10:13], force[listed]) and same(before[listed][:, 16:19], torque[listed])
    assert same(after_remove, before[keep])                              # all 38 doubles, the forces among them
    assert first == N - 5 and same(after_add, np.concatenate([before[keep], fresh]))


# ---- 3. map shapes ---------------------------------------------------------------------------------------------------------------
def check_removal(w, bodies, removed):
    want_map, keep = expected_map(len(bodies), removed)
    old_to_new, joint_map = w.remove_bodies(removed)
    assert same(old_to_new, want_map), removed
    assert joint_map.size == 0 and w.n == int(keep.sum())
    assert C.c_uint32(capi.hip_lib().xpbd_world_body_count(w._h)).value == w.n
    got = w.download()
    assert same(got, bodies[keep]), removed
    return keep


@pytest.mark.parametrize("removed", [[], [0], [N - 1], [63], [64], list(range(1, N)), list(range(N)), [7, 64, 7, 129, 64, 7]],
                         ids=["none", "first", "last", "63", "64", "all_but_one", "all", "duplicates"])
def test_map_shapes_on_the_small_world(removed):
    bodies, sid = scene(BOXES)
    with world(BOXES, bodies, sid, capi.MODE_FUSED) as w:
        keep = check_removal(w, bodies, np.array(removed, dtype=np.uint32))
        if not keep.any():                                               # a world of 0 bodies, as upload(.., 0) leaves it: it takes new bodies
            assert w.download().shape == (0, 38)
            assert w.add_bodies(bodies[:3], sid[:3]) == 0 and same(w.download(), bodies[:3])


@pytest.mark.parametrize("density", [0.01, 0.5, 0.99])
def test_map_of_random_flags_across_scan_blocks(density):
    n = 1300                                                             # more than one scan block (1024) and more than five gather blocks
    bodies, sid = pile(capi, BOXES, n, 3, 12.0, 12.0)
    rng = np.random.default_rng(int(density * 100))
    removed = np.flatnonzero(rng.uniform(size=n) < density).astype(np.uint32)
    assert 0 < removed.size < n
    with world(BOXES, bodies, sid, capi.MODE_FUSED) as w:
        check_removal(w, bodies, rng.permutation(removed))


def test_counts_that_move_the_stride_across_256():
    bodies, sid = pile(capi, BOXES, 258, 4, 6.0, 8.0)
    with world(BOXES, bodies[:257], sid[:257], capi.MODE_FUSED) as w:    # 257 (stride 512) -> 256 (stride 256) by removal
        check_removal(w, bodies[:257], np.array([100], dtype=np.uint32))
        kept = np.delete(bodies[:257], 100, axis=0)
        kept_sid = np.delete(sid[:257], 100)
        assert w.add_bodies(bodies[257:258], sid[257:258]) == 256        # 256 -> 257 (stride 512) by addition
        now = np.concatenate([kept, bodies[257:258]])
        assert same(w.download(), now)
        w.step(DT, SUBSTEPS)
        got = (w.download(), w.contacts())
    with world(BOXES, now, np.concatenate([kept_sid, sid[257:258]]), capi.MODE_FUSED) as f:
        f.step(DT, SUBSTEPS)
        assert same(got[0], f.download()) and same(got[1], f.contacts())


# ---- 4. the device variant -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_child(tmp_path_factory):
    """population_device_child.py, once: remove_bodies_device driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("population") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "population_device_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out)), json.loads(p.stdout.strip().splitlines()[-1])


def test_device_variant_equals_the_host_variant(device_child):
    res, _ = device_child
    bodies, sid = scene(BOXES)
    s = settings_for()
    with world(BOXES, bodies, sid) as w:
        apply_settings(w, s)
        w.step(DT, SUBSTEPS)
        old_to_new, joint_map = w.remove_bodies(REMOVED)
        changed = w.download()
        w.step(DT, SUBSTEPS)
        stepped = w.download()
    assert same(res["flags_map"], old_to_new) and same(res["flags_joint_map"], joint_map)
    assert same(res["flags_changed"], changed) and same(res["flags_stepped"], stepped)
    assert same(res["none_map"], np.arange(N, dtype=np.uint32)) and res["none_history"] == 1     # no flag set: nothing changes


def test_flags_built_from_an_overlap_result_on_the_stream(device_child):
    res, verdict = device_child
    assert 1 <= verdict["hits"] <= verdict["cap"]
    bodies, sid = scene(BOXES)
    with world(BOXES, bodies, sid) as w:
        w.step(DT, SUBSTEPS)
        offsets, hits = w.overlap(pc.trigger_volume())
        assert len(hits) == verdict["hits"]
        old_to_new, _ = w.remove_bodies(hits["body"])
        assert same(res["trigger_map"], old_to_new) and same(res["trigger_changed"], w.download())
        assert w.n == N - len(np.unique(hits["body"]))                    # (a body inside two of the volumes is listed twice)


# ---- 5. joints -------------------------------------------------------------------------------------------------------------------
def jointed_world(bodies, sid, joints, lims, drives):
    w = world(BOXES, bodies, sid)
    w.set_joints(joints)
    w.set_joint_limits(lims)
    w.set_joint_drives(drives)
    return w


def test_joints_follow_their_bodies_with_limits_and_drives():
    bodies, sid = scene(BOXES)
    s = settings_for()
    removed = np.array([43], dtype=np.uint32)                            # the end of hinge 20 (40-43), which has a limit and a drive
    want_map, keep = expected_map(N, removed)
    joints, lims, drives, want_joint_map = reindex_joints(s, want_map)
    assert len(joints) == len(s["joints"]) - 1 and len(lims) == len(s["lims"]) - 1 and len(drives) == len(s["drives"]) - 1
    assert (joints["body_a"] > joints["body_b"]).any()                   # the joint given the other way round keeps its orientation
    with jointed_world(bodies, sid, s["joints"], s["lims"], s["drives"]) as a:
        a.step(DT, SUBSTEPS)
        _, joint_map = a.remove_bodies(removed)
        changed = a.download()
        got = bc.stepped(a)
    assert same(joint_map, want_joint_map) and joint_map[20] == NO_HIT and joint_map[21] == 20
    with jointed_world(changed, sid[keep], joints, lims, drives) as b:
        want = bc.stepped(b)
    assert same(got[0], want[0]) and same(got[1], want[1])
    with world(BOXES, changed, sid[keep]) as free:                       # ... and the joints that stayed do act
        assert not same(bc.stepped(free)[0], want[0])


def test_a_world_whose_every_joint_is_dropped_steps_like_a_world_without_joints():
    bodies, sid = scene(BOXES)
    s = settings_for()
    few = s["joints"][[pc.HINGES[0], pc.SLIDERS[0]]].copy()               # 2-5 and 14-17
    lims = s["lims"][[1, 2]].copy()
    lims["joint"] = [0, 1]
    drives = s["drives"][[1, 0]].copy()
    drives["joint"] = [0, 1]
    removed = np.array([5, 14], dtype=np.uint32)
    _, keep = expected_map(N, removed)
    with jointed_world(bodies, sid, few, lims, drives) as a:
        a.step(DT, SUBSTEPS)
        _, joint_map = a.remove_bodies(removed)
        assert joint_map.tolist() == [NO_HIT, NO_HIT] and a.n_joints == 0
        changed = a.download()
        got = bc.stepped(a)
    with world(BOXES, changed, sid[keep]) as b:
        want = bc.stepped(b)
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---- 6. settings that stay off stay off ------------------------------------------------------------------------------------------
def test_a_world_without_settings_equals_a_fresh_world_that_never_set_them():
    bodies, sid = scene(MIXED)
    fresh, fresh_sid = newcomers(MIXED, N_ADD)
    _, keep = expected_map(N, REMOVED)
    with world(MIXED, bodies, sid) as a:
        a.set_contact_report(True)
        a.step(DT, SUBSTEPS)
        a.remove_bodies(REMOVED)
        a.add_bodies(fresh, fresh_sid)
        changed = a.download()
        got = pc.run(a, 3, True)
    with world(MIXED, changed, np.concatenate([sid[keep], fresh_sid])) as b:
        b.set_contact_report(True)
        want = pc.run(b, 3, True)
    assert same_runs(got, want)


def test_added_bodies_get_the_default_filter():
    bodies, sid = scene(BOXES)
    filters = np.zeros(N, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 2, 2
    lone = bodies[:1].copy()
    lone[0, 31:34] = [50.0, 50.0, 5.0]                                   # far from the pile
    lone[0, 34:38] = [1.0, 0.0, 0.0, 0.0]
    with world(BOXES, bodies, sid) as w:
        w.set_collision_filters(filters)
        first = w.add_bodies(lone, sid[:1])
        centre = lone[0, 31:34] + lone[0, 28:31]
        old = bodies[7, 31:34] + bodies[7, 28:31]
        rays = capi.rays([centre + [0.0, 0.0, 10.0], old + [0.0, 0.0, 30.0]], [[0.0, 0.0, -1.0]])
        masked = w.raycast(rays, mask=1)
        assert masked["body"][0] == first == N                           # group ~0 meets mask 1
        assert masked["body"][1] == NO_HIT                               # the pile is group 2: nothing answers mask 1
        assert w.raycast(rays, mask=2)["body"][1] != NO_HIT


# ---- 7. rejected calls change nothing --------------------------------------------------------------------------------------------
def joint_count(w):
    """The world's joint count through the ABI: n == 0 writes the identity over that many entries."""
    probe = np.full(512, 0xABABABAB, dtype=np.uint32)
    n = C.c_uint32(0)
    assert capi.hip_lib().xpbd_world_remove_bodies(w._h, None, 0, None, probe.ctypes.data, C.byref(n)) == capi.OK
    assert n.value == w.n
    return int(np.count_nonzero(probe != 0xABABABAB))


def test_rejected_calls_change_nothing_and_name_themselves():
    bodies, sid = scene(BOXES)
    s = settings_for()
    L = capi.hip_lib()
    p = lambda a: None if a is None else a.ctypes.data    # noqa: E731
    idx = np.array([3, N, 64], dtype=np.uint32)
    one, one_sid = newcomers(BOXES, 2)
    bad_sid = np.array([0, 99], dtype=np.uint32)
    out = C.c_uint32(12345)
    maps = np.full(N, 0xCDCDCDCD, dtype=np.uint32)
    rejected = {
        "remove: index == body count": ("xpbd_world_remove_bodies", lambda h: L.xpbd_world_remove_bodies(h, p(idx), 3, p(maps), p(maps), C.byref(out))),
        "remove: NULL indices with n > 0": ("xpbd_world_remove_bodies", lambda h: L.xpbd_world_remove_bodies(h, None, 3, p(maps), p(maps), C.byref(out))),
        "remove_device: NULL flags": ("xpbd_world_remove_bodies_device", lambda h: L.xpbd_world_remove_bodies_device(h, None, None, p(maps), C.byref(out))),
        "add: shape id out of range": ("xpbd_world_add_bodies", lambda h: L.xpbd_world_add_bodies(h, p(one), p(bad_sid), 2, C.byref(out))),
        "add: NULL aos": ("xpbd_world_add_bodies", lambda h: L.xpbd_world_add_bodies(h, None, p(one_sid), 2, C.byref(out))),
        "add: NULL shape ids": ("xpbd_world_add_bodies", lambda h: L.xpbd_world_add_bodies(h, p(one), None, 2, C.byref(out))),
        "add: more bodies than an upload accepts": ("xpbd_world_add_bodies", lambda h: L.xpbd_world_add_bodies(h, p(one), p(one_sid), 0xFFFFFFF0, C.byref(out))),
    }
    with world(BOXES, bodies, sid) as w, world(BOXES, bodies, sid) as twin:
        for x in (w, twin):
            apply_settings(x, s)
            x.step(DT, SUBSTEPS)
        assert w.history_push() == 0 and twin.history_push() == 0
        before = w.download()
        for what, (name, call) in rejected.items():
            assert call(w._h) == capi.E_INVALID, what
            assert L.xpbd_last_error().decode().startswith(name + ": "), (what, L.xpbd_last_error())
            assert out.value == 12345 and (maps == 0xCDCDCDCD).all(), what
            assert L.xpbd_world_body_count(w._h) == N and joint_count(w) == len(s["joints"]), what
            assert same(w.download(), before), what
        # n == 0 / n_add == 0 do nothing at all: the history stays
        old_to_new, joint_map = w.remove_bodies(np.zeros(0, dtype=np.uint32))
        assert same(old_to_new, np.arange(N, dtype=np.uint32)) and same(joint_map, np.arange(len(s["joints"]), dtype=np.uint32))
        assert w.add_bodies(np.zeros((0, 38)), np.zeros(0, dtype=np.uint32)) == N
        assert w.history_length() == 1
        w.history_restore(0)
        twin.history_restore(0)                                          # (a restore empties S_prev: the twin does the same)
        assert same(w.download(), before)
        got, want = pc.run(w, 1, True), pc.run(twin, 1, True)
        assert same_runs(got, want)                                      # bodies, reports against the same S_prev, neighbour lists
        # a real change empties the history
        w.history_push()
        w.remove_bodies(np.array([9], dtype=np.uint32))
        assert w.history_length() == 0
        with pytest.raises(capi.XpbdError) as e:
            w.history_restore(0)
        assert e.value.code == capi.E_INVALID
    with capi.World() as empty:                                          # a world without resident bodies
        empty.set_polytopes(capi.scene_polytopes(BOXES))
        assert L.xpbd_world_remove_bodies(empty._h, p(idx), 1, None, None, None) == capi.E_INVALID
        assert b"no bodies" in L.xpbd_last_error()
        flags = np.zeros(4, dtype=np.uint8)                              # (rejected before the pointer is looked at)
        assert L.xpbd_world_remove_bodies_device(empty._h, p(flags), None, None, None) == capi.E_INVALID


def test_an_added_body_is_checked_exactly_as_an_uploaded_one():
    """xpbd_world_upload_bodies checks the shape ids and takes the values of an xpbd_rigid as given (a singular inertia is an
    error of Rigid::new on the host mirror, not of the ABI): whatever it returns for a body, xpbd_world_add_bodies returns too."""
    bodies, sid = scene(BOXES)
    L = capi.hip_lib()
    singular = bodies[:2].copy()
    singular[1, 1:10] = 0.0                                              # a zero inverse inertia with a finite mass
    cases = {"singular inertia": (singular, sid[:2].copy()), "shape id out of range": (bodies[:2].copy(), np.array([0, 99], dtype=np.uint32))}
    with world(BOXES, bodies, sid) as w, world(BOXES, bodies, sid) as probe:
        count = N
        for what, (rows, ids) in cases.items():
            rc_upload = L.xpbd_world_upload_bodies(probe._h, rows.ctypes.data, ids.ctypes.data_as(C.POINTER(C.c_uint32)), 2)
            rc_add = L.xpbd_world_add_bodies(w._h, rows.ctypes.data, ids.ctypes.data, 2, None)
            assert rc_add == rc_upload, what
            count += 2 if rc_add == capi.OK else 0
            assert L.xpbd_world_body_count(w._h) == count, what
        assert count == N + 2                                            # the zero inertia was taken as upload takes it, the shape id refused


# ---- 8. repeated churn -----------------------------------------------------------------------------------------------------------
def test_twenty_rounds_of_churn_equal_a_twin_driven_through_upload():
    kind = MIXED
    bodies, sid = scene(kind)
    s = settings_for()
    pool, pool_sid = scene(kind, seed=123)
    rng = np.random.default_rng(17)
    with world(kind, bodies, sid) as a, world(kind, bodies, sid) as b:
        apply_settings(a, s, report=False)
        apply_settings(b, s, report=False)
        b_sid = sid.copy()
        for r in range(20):
            a.step(DT, SUBSTEPS)
            b.step(DT, SUBSTEPS)
            removed = rng.choice(a.n, 5, replace=False).astype(np.uint32)
            fresh, fresh_sid = pool[5 * r:5 * r + 5].copy(), pool_sid[5 * r:5 * r + 5]
            fresh[:, 33] += 6.0
            # A: the new calls
            old_to_new, _ = a.remove_bodies(removed)
            assert a.add_bodies(fresh, fresh_sid) == N - 5
            # B: download, numpy edit, upload, every setting again -- re-indexed by the test
            want_map, keep = expected_map(N, removed)
            assert same(old_to_new, want_map)
            state = np.concatenate([b.download()[keep], fresh])
            b_sid = np.concatenate([b_sid[keep], fresh_sid])
            s = reindex_settings(s, want_map, 5)
            b.upload(state, b_sid)
            apply_settings(b, s, report=False)
            assert same(a.download(), state), r
        got, want = pc.run(a, 2, False), pc.run(b, 2, False)
        assert same_runs(got, want)
        assert same_runs(list(a.neighbours(DT)), list(b.neighbours(DT)))
