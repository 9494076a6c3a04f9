"""Contact islands (xpbd_world_islands, xpbd_world_islands_device) on the GPU against the independent model
(islands_model.py).  Every comparison is exact: integers equal, doubles bit-equal.  The grouping's loop cap is never expected
to trigger: the tests only ever see XPBD_OK from a well-formed call."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import islands_common as ic
import islands_model as im
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DT = ic.DT
NONE = capi.ISLAND_NONE
NO_JOINTS, NO_CONTACTS = capi.ISLANDS_NO_JOINTS, capi.ISLANDS_NO_CONTACTS


def rows(records, *fields):
    return [tuple(int(r[f]) for f in fields) for r in records]


# ---- 1. graphs without stepping: joints only --------------------------------------------------------------------------------------
def chain_with_gaps(n):
    a = np.array([i for i in range(n - 1) if i % 7 != 6], dtype=np.uint32)
    return ic.distance_joints(a, a + 1)


def permuted_chain(n, seed):
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    j = ic.distance_joints(order[:-1], order[1:])
    return j[rng.permutation(len(j))]


def star(n, hub):
    leaves = np.array([i for i in range(n) if i != hub], dtype=np.uint32)
    j = ic.distance_joints(np.full(len(leaves), hub), leaves)
    flip = np.arange(len(j)) % 3 == 1                        # both orientations of a joint
    j["body_a"][flip], j["body_b"][flip] = leaves[flip], hub
    return j


GRAPHS = {
    "n=1": lambda: (1, ic.distance_joints([], []), ()),
    "n=63": lambda: (63, chain_with_gaps(63), ()),
    "n=64": lambda: (64, chain_with_gaps(64), ()),
    "n=65": lambda: (65, chain_with_gaps(65), ()),
    "chain 4096 ascending": lambda: (4096, ic.distance_joints(np.arange(4095), np.arange(1, 4096)), ()),
    "chain 4096 permuted": lambda: (4096, permuted_chain(4096, 20240607), ()),
    "star on body 0": lambda: (4096, star(4096, 0), ()),
    "star on the largest index": lambda: (4096, star(4096, 4095), ()),
    "star with a fixed hub": lambda: (4096, star(4096, 0), (0,)),
    "512 disjoint pairs": lambda: (1024, ic.distance_joints(np.arange(0, 1024, 2), np.arange(1, 1024, 2)), ()),
    "zero joints": lambda: (100, ic.distance_joints([], []), ()),
    "duplicate joints": lambda: (3, ic.distance_joints([0, 2, 0], [2, 0, 2]), ()),
}
# what each graph must give: island count, and (first_body, n_bodies, n_joints, n_anchors) of its first island
EXPECTED = {
    "n=1": (1, (0, 1, 0, 0)), "n=63": (9, (0, 7, 6, 0)), "n=64": (10, (0, 7, 6, 0)), "n=65": (10, (0, 7, 6, 0)),
    "chain 4096 ascending": (1, (0, 4096, 4095, 0)), "chain 4096 permuted": (1, (0, 4096, 4095, 0)),
    "star on body 0": (1, (0, 4096, 4095, 0)), "star on the largest index": (1, (0, 4096, 4095, 0)),
    "star with a fixed hub": (4095, (1, 1, 0, 1)), "512 disjoint pairs": (512, (0, 2, 1, 0)), "zero joints": (100, (0, 1, 0, 0)),
    "duplicate joints": (2, (0, 2, 3, 0)),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_joint_graphs_without_stepping(name):
    n, joints, fixed = GRAPHS[name]()
    bodies, sid = ic.spread_bodies(n, fixed=fixed)
    if n == 65:
        bodies[40, 22] = np.nan                              # a NaN velocity shows as a NaN in its island's record
    with ic.graph_world(bodies, sid, joints) as w:
        island_of, got = ic.assert_equals_model(w, joints, NO_CONTACTS)
    count, first = EXPECTED[name]
    assert len(got) == count and rows(got[:1], "first_body", "n_bodies", "n_joints", "n_anchors") == [first]
    assert not got["n_pairs"].any() and not got["n_grounded"].any()       # nothing was stepped, contacts do not count
    assert int(got["n_bodies"].sum()) == n - len(fixed) and np.all(np.diff(got["first_body"].astype(np.int64)) > 0)
    if name == "star with a fixed hub":
        assert island_of[0] == NONE and np.array_equal(island_of[1:], np.arange(4095, dtype=np.uint32))
        assert np.all(got["n_bodies"] == 1) and np.all(got["n_anchors"] == 1) and not got["n_joints"].any()
    if n == 65:
        assert np.isnan(got["max_speed2"][island_of[40]]) and int(np.isnan(got["max_speed2"]).sum()) == 1


# ---- 2. a crafted scene, stepped with reports on ------------------------------------------------------------------------------------
def test_crafted_scene_gives_the_islands_written_down_here():
    w, joints = ic.crafted_world()
    with w:
        for _ in range(6):
            w.step(DT, 20)
        island_of, got = ic.assert_equals_model(w, joints, 0)
        pairs = w.pair_contacts(points=False)[0]
        for flags in (NO_JOINTS, NO_CONTACTS):
            ic.assert_equals_model(w, joints, flags)
    print("touching pairs:", [(int(a), int(b)) for a, b in zip(pairs["body_a"], pairs["body_b"])])
    print("islands:", rows(got, *got.dtype.names[:6]))
    assert island_of.tolist() == [0, 0, 0, 1, 1, 1, NONE, 2, 3, NONE, 4, 4, 4, 4, 4, 5]
    #                 first_body, n_bodies, n_pairs, n_joints, n_anchors, n_grounded
    assert rows(got, *got.dtype.names[:6]) == [(0, 3, 2, 0, 0, 1), (3, 3, 2, 0, 0, 1),          # the stacks: the bottom box is on the ground
                                               (7, 1, 0, 0, 1, 0), (8, 1, 0, 0, 1, 0),          # apart on one slab: two islands, one anchor each
                                               (10, 5, 0, 4, 1, 0),                             # the chain: four joints inside, one to the post
                                               (15, 1, 0, 0, 0, 0)]                             # free fall
    assert got["max_speed2"][5] > 0.25                       # 0.1 s of free fall is about 1 m/s


# ---- 3. a 512-box drop, a few frames in ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
def test_box_drop_equals_the_model_for_every_flag(narrowphase):
    w, joints = ic.drop_world(narrowphase, fixed=(5, 200))
    with w:
        for _ in range(60):                                  # one second: the second layer has fallen its 1.5 m onto the first
            w.step(DT, 10)
        n_pairs = w.contact_report_counts()[0]
        island_of, got = ic.assert_equals_model(w, joints, 0)
        _, contacts_only = ic.assert_equals_model(w, joints, NO_JOINTS)
        _, joints_only = ic.assert_equals_model(w, joints, NO_CONTACTS)
    print("pairs %d, joints %d, islands %d / %d / %d, largest %d" % (n_pairs, len(joints), len(got), len(contacts_only), len(joints_only),
                                                                    int(got["n_bodies"].max())))
    assert n_pairs > 50 and len(joints) > 20                 # the pile has landed on itself, and some boxes carry joints
    assert int(got["n_pairs"].sum() + got["n_anchors"].sum()) <= n_pairs + len(joints)
    assert got["n_bodies"].max() >= 3 and got["n_grounded"].sum() > 50
    assert len(got) < len(contacts_only) and len(got) < len(joints_only) <= 510
    assert island_of[5] == NONE and island_of[200] == NONE


# ---- 4. the device call ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_child(tmp_path_factory):
    """islands_device_child.py, once: xpbd_world_islands_device driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("islands") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "islands_device_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out)), json.loads(p.stdout.strip().splitlines()[-1])


def test_device_call_gives_the_host_calls_bits(device_child):
    res, verdict = device_child
    total = int(res["host_total"])
    assert total == verdict["total"] and total > 8
    for flags in (0, NO_JOINTS, NO_CONTACTS):
        tag = "f%d_" % flags
        assert int(res[tag + "device_total"]) == int(res[tag + "host_total"])
        assert im.same_bytes(res[tag + "device_island_of"], res[tag + "host_island_of"])
        k = int(res[tag + "host_total"])
        assert im.same_bytes(res[tag + "device_records"][:k], res[tag + "host_records"])
        assert np.all(res[tag + "device_records"][k:].view(np.uint8) == 0x5A)     # nothing written past the total


def test_device_call_with_a_short_buffer_leaves_the_rest_untouched(device_child):
    res, verdict = device_child
    cap, total = verdict["short_cap"], int(res["host_total"])
    assert 0 < cap < total and int(res["short_total"]) == total
    assert im.same_bytes(res["short_records"][:cap], res["host_records"][:cap])
    assert np.all(res["short_records"][cap:].view(np.uint8) == 0x5A)
    assert im.same_bytes(res["short_island_of"], res["host_island_of"])
    assert int(res["count_only_total"]) == total                                   # no records, no island_of: the count alone


def test_device_flags_compose_with_remove_bodies_device(device_child):
    """"remove every island that has come to rest" without a host round trip: the child built the flags from the device call's
    outputs with torch, the parent checks the survivors against the host call's records."""
    res, verdict = device_child
    resting = np.flatnonzero((res["host_records"]["max_speed2"] < verdict["rest_speed2"])
                             & (res["host_records"]["max_angular_speed2"] < verdict["rest_speed2"]))
    gone = np.isin(res["host_island_of"], resting)
    assert 0 < gone.sum() < len(gone) and int(res["after_removal_count"]) == len(gone) - gone.sum()
    assert im.same_bytes(res["removal_map"] != NONE, ~gone)


# ---- 5. read-only ---------------------------------------------------------------------------------------------------------------------
def snapshot(w):
    pairs, points = w.pair_contacts()
    return [w.download(), w.contacts(), pairs, points, w.contact_events(), np.array(w.contact_report_counts())]


def test_a_call_changes_nothing_it_reads():
    w, _ = ic.drop_world()
    with w:
        for _ in range(60):
            w.step(DT, 10)
        before = snapshot(w)
        for flags in (0, NO_JOINTS, NO_CONTACTS):
            w.islands(flags)
        after = snapshot(w)
    assert len(before[2]) > 20
    assert all(im.same_bytes(a, b) for a, b in zip(before, after))


def test_a_world_that_calls_every_frame_ends_bit_equal_to_a_twin_that_never_does():
    a, _ = ic.drop_world()
    b, _ = ic.drop_world()
    with a, b:
        for _ in range(55):
            a.step(DT, 10)
            b.step(DT, 10)
        for _ in range(5):
            a.step(DT, 10)
            a.islands(0)                                     # before any report call: the islands compact the frame's keys
            b.step(DT, 10)
        ends = [snapshot(a), snapshot(b)]
    assert len(ends[0][2]) > 20
    assert all(im.same_bytes(x, y) for x, y in zip(*ends))


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def raw_call(w, flags, island_of, records, cap, total):
    p = lambda a: None if a is None else a.ctypes.data
    return capi.hip_lib().xpbd_world_islands(w._h, flags, p(island_of), p(records), cap, None if total is None else C.byref(total))


def test_errors():
    L = capi.hip_lib()
    total = C.c_uint32(77)
    records = np.zeros(16, dtype=capi.ISLAND_DTYPE)
    w, joints = ic.crafted_world(report=False)
    with w:
        island_of = np.zeros(w.n, dtype=np.uint32)
        # reports off: the contact edges are not there; the joints alone are
        assert raw_call(w, 0, island_of, records, 16, total) == capi.E_INVALID and b"reports are off" in L.xpbd_last_error()
        assert raw_call(w, NO_JOINTS, island_of, records, 16, total) == capi.E_INVALID
        assert raw_call(w, NO_CONTACTS, island_of, records, 16, total) == capi.OK and total.value == 10
        total.value = 77
        w.set_contact_report(True)
        # before any step
        assert raw_call(w, 0, island_of, records, 16, total) == capi.E_INVALID and b"no report" in L.xpbd_last_error()
        w.history_push()
        w.step(DT, 4)
        assert raw_call(w, 0, island_of, records, 16, total) == capi.OK and 6 <= total.value <= 10
        # unknown flags, both flags, NULLs
        total.value = 77
        assert raw_call(w, 4, island_of, records, 16, total) == capi.E_INVALID and b"unknown flags" in L.xpbd_last_error()
        assert raw_call(w, NO_JOINTS | NO_CONTACTS, island_of, records, 16, total) == capi.E_INVALID
        assert raw_call(w, 0, island_of, records, 16, None) == capi.E_INVALID
        assert raw_call(w, 0, island_of, None, 16, total) == capi.E_INVALID
        assert L.xpbd_world_islands(None, 0, None, None, 0, C.byref(total)) == capi.E_INVALID
        assert L.xpbd_world_islands_device(None, 0, None, None, 0, None) == capi.E_INVALID
        assert L.xpbd_world_islands_device(w._h, 0, None, None, 0, None) == capi.E_INVALID
        assert L.xpbd_world_islands_device(w._h, 8, None, None, 0, None) == capi.E_INVALID
        assert total.value == 77
        # NULL outputs that are allowed: no island_of; no records with cap 0 (more than nothing is a capacity error)
        assert raw_call(w, NO_CONTACTS, None, records, 16, total) == capi.OK and total.value == 10
        assert raw_call(w, NO_CONTACTS, None, None, 0, total) == capi.E_CAPACITY and total.value == 10
        # XPBD_E_CAPACITY: the first cap records filled, the total reported
        _, full = w.islands(NO_CONTACTS)
        short = np.zeros(16, dtype=capi.ISLAND_DTYPE)
        short.view(np.uint8)[:] = 0x5A
        total.value = 0
        assert raw_call(w, NO_CONTACTS, island_of, short, 3, total) == capi.E_CAPACITY and total.value == 10
        assert b"10 islands, capacity 3" in L.xpbd_last_error()
        assert im.same_bytes(short[:3], full[:3]) and np.all(short[3:].view(np.uint8) == 0x5A)
        # after a history restore the report is gone
        w.history_restore(0)
        assert raw_call(w, 0, island_of, records, 16, total) == capi.E_INVALID and b"no report" in L.xpbd_last_error()
        assert raw_call(w, NO_CONTACTS, island_of, records, 16, total) == capi.OK
    with capi.World(mode=capi.MODE_CONTACTS) as empty:       # no resident bodies
        assert raw_call(empty, NO_CONTACTS, None, records, 16, total) == capi.E_INVALID and b"no bodies" in L.xpbd_last_error()


# ---- 7. population --------------------------------------------------------------------------------------------------------------------
def test_after_remove_bodies_the_islands_are_those_of_the_reindexed_world():
    w, joints = ic.drop_world(fixed=(5, 200))
    removed = np.array([0, 1, 7, 64, 65, 66, 130, 200, 333, 511], dtype=np.uint32)
    with w:
        for _ in range(4):
            w.step(DT, 10)
        old_to_new, joint_map = w.remove_bodies(removed)
        kept = joints[joint_map != capi.NO_HIT].copy()
        kept["body_a"], kept["body_b"] = old_to_new[kept["body_a"]], old_to_new[kept["body_b"]]
        assert w.n == 502 and 0 < len(kept) < len(joints)
        island_of, got = ic.assert_equals_model(w, kept, NO_CONTACTS)
        total = C.c_uint32(0)
        assert raw_call(w, 0, None, None, 0, total) == capi.E_INVALID       # the report's frame went with the old population
    assert island_of[old_to_new[5]] == NONE and not got["n_grounded"].any() and len(got) <= 501
    assert int(got["n_joints"].sum() + got["n_anchors"].sum()) == len(kept)     # every surviving joint counts exactly once
