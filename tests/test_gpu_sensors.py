"""Sensor bodies (include/xpbd.h, "SENSOR bodies") on the GPU.  A sensor pair is reported and never solved, so world A (sensors
flagged) steps bit for bit like world B (the same bodies filtered out with {group 0, mask 0}) while a control C (neither) does
not; its report holds the sensor pairs as the oracle's SAT gives them; events, occupancy, islands, sleeping and the table's
lifetime follow the header.  Every comparison is on bytes or integers."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import contact_report_model as rm
import oracle_binding as ob
import sensor_common as sc
import sensor_model as sm
import sleep_common as slc
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DT = sc.DT
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
FRAMES, SUBSTEPS = 5, 4


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pair_list(w):
    """The current frame's pair list, from the neighbour lists of its broadphase (no new broadphase)."""
    off, nb = w.frame_neighbours()
    return rm.upper_pairs(off, nb), off, nb


def run(w, frames=FRAMES, substeps=SUBSTEPS):
    out = []
    for _ in range(frames):
        w.step(DT, substeps)
        out.append(sc.Frame(w, substeps))
    return out


# ---- 1. pass-through equals the filtered world ---------------------------------------------------------------------------------
@pytest.mark.parametrize("materials", [False, True], ids=["plain", "materials"])
@pytest.mark.parametrize("schedule", ["fused", "kinematic", "restitution"])
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA], ids=["sat", "gjk"])
def test_a_world_with_sensors_steps_like_the_world_that_filters_them_out(narrowphase, schedule, materials):
    """fused: the fused contacts schedule (no restitution; the fourth fixed sensor stands still, because a kinematic table selects
    the unfused schedule); kinematic: the same with that sensor moving through the clump; restitution: the unfused schedule with
    the velocity pass, the sensor moving."""
    bodies, sid, is_sensor, table = sc.clump_scene("fixed" if schedule == "fused" else "kinematic")
    frames = {}
    for kind in "ABC":
        with sc.make_world(kind, sc.mixed_polytopes(), bodies, sid, is_sensor, narrowphase, schedule == "restitution", materials, table) as w:
            frames[kind] = run(w)
            if kind == "A":
                pairs = w.pair_contacts(points=False)[0]
                stats = w.contact_stats()
                assert w.sensor_count() == int(is_sensor.sum())
    for f in range(FRAMES):
        assert frames["A"][f].same(frames["B"][f]), f
    assert not frames["A"][-1].same(frames["C"][-1])
    touching = pairs[sc.sensor_pairs(pairs, is_sensor) & (pairs["n_points"] > 0)]
    print("sensor pairs touching in the last frame:", len(touching), "of", len(pairs), "records; stats", stats)
    assert len(touching) >= 30
    assert stats[0] >= len(pairs)          # the pair count includes the sensor pairs


# ---- 2. the wave-wide "at most two neighbours" shortcut, eight lanes and one lane per body ---------------------------------------
@pytest.mark.parametrize("cells", [512, 6720], ids=["512_boxes", "20160_bodies"])
def test_the_two_neighbour_shortcut_skips_the_sensor(cells):
    """64 k boxes, every one with its own floor and its own sensor, so that whole waves of the pair solve hold bodies with exactly
    two neighbours: 512 boxes (1 536 bodies: eight lanes per body) and 6 720 boxes (20 160 bodies, above the small-world limit: one
    lane per body)."""
    bodies, sid, is_sensor = sc.cells_scene(cells)
    assert (len(bodies) > SMALL_WORLD) == (cells == 6720)
    frames = {}
    for kind in "ABC":
        with sc.make_world(kind, sc.box_polytopes(), bodies, sid, is_sensor) as w:
            frames[kind] = run(w)
            if kind == "A":
                off, _ = w.frame_neighbours()
                pairs = w.pair_contacts(points=False)[0]
    assert np.all(np.diff(off.astype(np.int64))[:cells] == 2) and np.all(np.diff(off.astype(np.int64))[cells:] == 1)
    for f in range(FRAMES):
        assert frames["A"][f].same(frames["B"][f]), f
    assert not frames["A"][-1].same(frames["C"][-1])
    probes = pairs[sc.sensor_pairs(pairs, is_sensor)]
    assert len(probes) == cells and np.all(probes["n_points"] > 0) and np.all(probes["substeps"] == SUBSTEPS)
    assert len(pairs) == 2 * cells


# ---- 3. the report ---------------------------------------------------------------------------------------------------------------
def test_sensor_pairs_are_reported_as_the_oracle_sat_gives_them():
    bodies, sid, is_sensor, _ = sc.clump_scene("fixed")
    polys = ob.polytopes_array(sc.MIXED_NAMES)
    substeps = 3
    h = DT / substeps
    reports = {}
    for kind in "AB":
        with sc.make_world(kind, sc.mixed_polytopes(), bodies, sid, is_sensor, trace=False) as w:
            w.step(DT, substeps)                     # a frame of settling first
            w.contacts_begin(DT)
            if kind == "A":
                pairs, _, _ = pair_list(w)
                counts = {}
            for k in range(substeps):
                if kind == "A":
                    frames = rm.p1_frames(w.download(), h)
                    touching = rm.manifolds(frames, sid, polys, pairs)
                    for key in touching:
                        counts[key] = counts.get(key, 0) + 1
                w.contacts_substep(h)
            reports[kind] = w.pair_contacts()
    got, points = reports["A"]
    keys = [(int(a), int(b)) for a, b in zip(got["body_a"], got["body_b"])]
    assert keys == sorted(counts) and [int(s) for s in got["substeps"]] == [counts[k] for k in keys]
    checked = 0
    for r, key in zip(got, keys):
        if not (is_sensor[key[0]] or is_sensor[key[1]]) or key not in touching:
            continue
        feature, npts, normal, depth, ref, inc = rm.record(frames, sid, polys, key[0], key[1], touching[key])
        assert (int(r["feature"]), int(r["n_points"])) == (feature, npts), key
        assert np.asarray(r["normal"], dtype=np.float64).tobytes() == np.asarray(normal, dtype=np.float64).tobytes(), key
        assert float(r["depth"]).hex() == float(depth).hex(), key
        p = points[r["first_point"]:r["first_point"] + npts]
        assert p["p_ref"].tobytes() == np.asarray(ref, dtype=np.float64).tobytes() and p["p_inc"].tobytes() == np.asarray(inc, dtype=np.float64).tobytes(), key
        checked += 1
    both = [k for k in keys if is_sensor[k[0]] and is_sensor[k[1]]]
    print("sensor records checked against the model:", checked, "sensor-sensor records:", len(both))
    assert checked >= 30 and len(both) >= 1
    # A's report without the sensor pairs is B's report
    solid = ~sc.sensor_pairs(got, is_sensor)
    want, want_points = reports["B"]
    assert same_bytes(sc.rebased(got[solid]), want) and len(want) > 50
    kept = np.concatenate([np.arange(r["first_point"], r["first_point"] + r["n_points"]) for r in got[solid]] or [np.zeros(0)]).astype(np.int64)
    assert same_bytes(points[kept], want_points)


# ---- 4. events by hand -------------------------------------------------------------------------------------------------------------
def test_a_box_falls_through_a_sensor_slab_with_begin_and_end():
    """Body 0: a box dropped from z = 5; body 1: a fixed sensor box at z in [2, 3].  The twin world holds the box alone."""
    substeps, frames = 4, 75
    h = DT / substeps
    bodies = np.concatenate([sc.cube_rows([[0.2, 0.1, 5.0]], fixed=False), sc.cube_rows([[0.0, 0.0, 2.0]], fixed=True)])
    sid = np.zeros(2, dtype=np.uint32)
    polys = ob.polytopes_array([("cube", 1.0)])
    begins, ends, prev = [], [], []
    with sc.make_world("A", [capi.polytope(capi.SHAPE_CUBE)], bodies, sid, np.array([0, 1], dtype=np.uint8), trace=False) as w, \
            sc.make_world("C", [capi.polytope(capi.SHAPE_CUBE)], bodies[:1], sid[:1], None, trace=False) as twin:
        for f in range(frames):
            w.contacts_begin(DT)
            twin.contacts_begin(DT)
            pairs, _, _ = pair_list(w)
            touched = False
            for _ in range(substeps):
                if pairs:
                    touched = touched or bool(rm.manifolds(rm.p1_frames(w.download(), h), sid, polys, pairs))
                w.contacts_substep(h)
                twin.contacts_substep(h)
            cur = [(0, 1)] if touched else []
            events = [tuple(int(v) for v in e) for e in w.contact_events()]
            assert events == rm.events(prev, cur), f
            begins += [f for e in events if e[2] == capi.CONTACT_BEGIN]
            ends += [f for e in events if e[2] == capi.CONTACT_END]
            prev = cur
            assert w.download()[0].tobytes() == twin.download()[0].tobytes(), f
        z = w.download()[0, 33]
    print("BEGIN in frames", begins, "END in frames", ends, "final z", z)
    assert len(begins) == 1 and len(ends) == 1 and 20 < begins[0] < ends[0] and z < 0.5


# ---- 5. occupancy ------------------------------------------------------------------------------------------------------------------
def assert_occupancy_equals_model(w, is_sensor):
    sensors, offsets, hits = w.sensor_overlaps()
    pairs = w.pair_contacts(points=False)[0]
    want = sm.occupancy(pairs["body_a"], pairs["body_b"], is_sensor)
    assert same_bytes(sensors, want[0]) and same_bytes(offsets, want[1]) and same_bytes(hits, want[2].astype(capi.SENSOR_HIT_DTYPE))
    return sensors, offsets, hits


def test_occupancy_equals_the_model_over_the_downloaded_records():
    w, is_sensor = sc.occupancy_world()
    with w:
        sensors, offsets, hits = assert_occupancy_equals_model(w, is_sensor)
        off, nb = w.frame_neighbours()
        per = dict(zip(sensors.tolist(), np.diff(offsets.astype(np.int64)).tolist()))
        assert per[sc.LONELY] == 0 and off[sc.LONELY + 1] == off[sc.LONELY]                 # no neighbours
        assert per[sc.MISSED] == 0 and off[sc.MISSED + 1] - off[sc.MISSED] == 1             # a neighbour that misses
        assert per[sc.CLUMP] > 20 and len(hits) > 100
        # a capacity below the total: offsets complete, the prefix filled, the total reported
        cap = len(hits) // 2
        rc, s2, o2, h2, total = w.sensor_overlaps_raw(cap)
        assert rc == capi.E_CAPACITY and total == len(hits) and same_bytes(s2, sensors) and same_bytes(o2, offsets) and same_bytes(h2, hits[:cap])
        rc, _, o3, _, total = w.sensor_overlaps_raw(0)
        assert rc == capi.E_CAPACITY and total == len(hits) and same_bytes(o3, offsets)
        # all bodies sensors
        w.set_sensors(np.ones(w.n, dtype=np.uint8))
        assert_occupancy_equals_model(w, np.ones(w.n, dtype=np.uint8))                      # the frame that is there
        w.step(DT, sc.OCC_SUBSTEPS)
        s4, o4, h4 = assert_occupancy_equals_model(w, np.ones(w.n, dtype=np.uint8))
        assert len(s4) == w.n and len(h4) == 2 * w.contact_report_counts()[0]
        # clearing the table
        w.set_sensors(None)
        L = capi.hip_lib()
        out, n_out = np.zeros(4, dtype=np.uint32), C.c_uint32(0)
        assert L.xpbd_world_sensor_overlaps(w._h, out.ctypes.data, out.ctypes.data, None, 0, C.byref(n_out)) == capi.E_INVALID
        assert b"no sensor" in L.xpbd_last_error()
        assert w.sensor_count() == 0 and not w.get_sensors().any()


@pytest.fixture(scope="module")
def device_child(tmp_path_factory):
    """sensor_device_child.py, once: xpbd_world_sensor_overlaps_device driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("sensors") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "sensor_device_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out)), json.loads(p.stdout.strip().splitlines()[-1])


def test_device_call_gives_the_host_calls_bits(device_child):
    res, verdict = device_child
    total = int(res["host_offsets"][-1])
    assert total == verdict["total"] and total > 100
    assert same_bytes(res["device_sensors"], res["host_sensors"]) and same_bytes(res["device_offsets"], res["host_offsets"])
    assert same_bytes(res["device_hits"][:total], res["host_hits"])
    fill = np.array([verdict["fill"]], dtype=np.uint32)[0]
    assert np.all(res["device_hits"][total:]["body"] == fill)                              # nothing written behind the total
    cap = verdict["short_cap"]
    assert same_bytes(res["short_offsets"], res["host_offsets"]) and same_bytes(res["short_hits"][:cap], res["host_hits"][:cap])
    bodies, sid, is_sensor = sc.occupancy_scene()
    want = sm.occupancy(res["pairs"]["body_a"], res["pairs"]["body_b"], is_sensor)
    assert same_bytes(res["host_hits"], want[2].astype(capi.SENSOR_HIT_DTYPE))
    k = int(np.flatnonzero(res["host_sensors"] == sc.CLUMP)[0])
    assert same_bytes(res["zone"], res["host_hits"]["body"][res["host_offsets"][k]:res["host_offsets"][k + 1]])


# ---- 6. islands ----------------------------------------------------------------------------------------------------------------------
def test_sensor_pairs_are_no_edges_of_the_islands():
    bodies, sid, is_sensor, _ = sc.clump_scene("fixed")
    got = {}
    for kind in "AB":
        with sc.make_world(kind, sc.mixed_polytopes(), bodies, sid, is_sensor, trace=False) as w:
            for _ in range(3):
                w.step(DT, SUBSTEPS)
            got[kind] = [w.islands(flags) for flags in (0, capi.ISLANDS_NO_JOINTS, capi.ISLANDS_NO_CONTACTS)]
            if kind == "A":
                pairs = w.pair_contacts(points=False)[0]
    for a, b in zip(got["A"], got["B"]):
        assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    assert int(sc.sensor_pairs(pairs, is_sensor).sum()) >= 30 and int(got["A"][0][1]["n_pairs"].sum()) > 50
    assert int(got["A"][2][1]["n_pairs"].sum()) == 0 and int(got["A"][2][1]["n_anchors"].sum()) == 0


# ---- 7. sleeping ---------------------------------------------------------------------------------------------------------------------
STACKS, HIGH, ZONE = 64, 4, 20.0


def stacks_scene():
    """64 four-high stacks of unit boxes (bodies 0..255, stack s = bodies 4 s .. 4 s + 3) 2 m apart on the ground, inside one fixed
    sensor box of edge 20 (body 256)."""
    at = [[2.0 * (s % 8), 2.0 * (s // 8), k * (1.0 + sc.GAP)] for s in range(STACKS) for k in range(HIGH)]
    bodies = np.concatenate([sc.cube_rows(at, fixed=False), sc.cube_rows([[-2.0, -2.0, -1.0]], fixed=True)])
    sid = np.concatenate([np.zeros(STACKS * HIGH), [1]]).astype(np.uint32)
    is_sensor = np.zeros(len(bodies), dtype=np.uint8)
    is_sensor[-1] = 1
    return bodies, sid, is_sensor


def test_a_stack_that_falls_asleep_inside_a_sensor_stays_listed():
    bodies, sid, is_sensor = stacks_scene()
    zone = len(bodies) - 1
    polytopes = [capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, ZONE)]
    worlds = {kind: sc.make_world(kind, polytopes, bodies, sid, is_sensor, trace=False) for kind in "AB"}
    try:
        for w in worlds.values():
            w.set_sleeping(*slc.CFG)
        a, b = worlds["A"], worlds["B"]
        asleep_frames = 0
        for f in range(slc.CFG[2] + 12):
            a.step(DT, slc.SUBSTEPS)
            b.step(DT, slc.SUBSTEPS)
            sa, sb = a.sleep_state(), b.sleep_state()
            assert all(same_bytes(x, y) for x, y in zip(sa[:3], sb[:3])) and sa[3] == sb[3], f
            assert a.download().tobytes() == b.download().tobytes(), f
            sensors, offsets, hits = a.sensor_overlaps()
            assert sensors.tolist() == [zone] and hits["body"].tolist() == list(range(STACKS * HIGH)), f
            events = a.contact_events()
            ends = events[events["kind"] == capi.CONTACT_END]
            assert not np.any((ends["body_a"] == zone) | (ends["body_b"] == zone)), f
            asleep_frames += int(sa[3][0] == STACKS * HIGH)
        print("frames with all", STACKS * HIGH, "boxes asleep and listed:", asleep_frames)
        assert asleep_frames >= 3
        # flagging a body wakes everybody
        flags = is_sensor.copy()
        flags[0] = 1
        a.set_sensors(flags)
        a.step(DT, slc.SUBSTEPS)
        asleep, rest, _, counts = a.sleep_state()
        assert counts[0] == 0 and not asleep.any() and int(rest.max()) <= 1
    finally:
        for w in worlds.values():
            w.close()


# ---- 8. lifetime ---------------------------------------------------------------------------------------------------------------------
def test_the_table_follows_population_changes_and_an_upload_clears_it():
    bodies, sid, is_sensor, _ = sc.clump_scene("fixed")
    gone = [5, 10, 17, 40, sc.CLUMP]              # 10 and 40: dynamic sensors; 300: a big fixed sensor; 5, 17: occupants
    new_rows = sc.cube_rows([[0.3, 0.2, 2.5], [8.0, 8.0, 1.0], [-0.4, 0.1, 3.1]], fixed=False)
    with sc.make_world("A", sc.mixed_polytopes(), bodies, sid, is_sensor) as w:
        run(w, 2)
        old_to_new, _ = w.remove_bodies(gone)
        keep = np.setdiff1d(np.arange(len(bodies)), gone)
        assert same_bytes(w.get_sensors(), is_sensor[keep]) and w.sensor_count() == int(is_sensor[keep].sum())
        first = w.add_bodies(new_rows, np.zeros(3, dtype=np.uint32))
        table = np.concatenate([is_sensor[keep], np.zeros(3, dtype=np.uint8)])
        assert first == len(keep) and same_bytes(w.get_sensors(), table) and w.sensor_count() == int(table.sum())
        state, sid_now = w.download(), np.concatenate([sid[keep], np.zeros(3, dtype=np.uint32)]).astype(np.uint32)
        after = run(w, 3)
        occupants = w.sensor_overlaps()
        # an upload clears the table
        w.upload(state, sid_now)
        assert w.sensor_count() == 0 and not w.get_sensors().any()
    with sc.make_world("A", sc.mixed_polytopes(), state, sid_now, table) as fresh:
        want = run(fresh, 3)
        want_occupants = fresh.sensor_overlaps()
    for f in range(3):
        assert after[f].same(want[f]), f
    assert all(same_bytes(x, y) for x, y in zip(occupants, want_occupants)) and len(occupants[2]) > 50


def test_a_cleared_table_steps_like_a_world_that_never_had_one():
    bodies, sid, is_sensor, _ = sc.clump_scene("fixed")
    with sc.make_world("A", sc.mixed_polytopes(), bodies, sid, is_sensor) as w, sc.make_world("C", sc.mixed_polytopes(), bodies, sid, is_sensor) as c:
        w.set_sensors(None)
        got, want = run(w, 3), run(c, 3)
        w.set_sensors(np.zeros(len(bodies), dtype=np.uint8))           # all zero: nothing flagged, the same again
        got += run(w, 2)
        want += run(c, 2)
    assert all(g.same(x) for g, x in zip(got, want))
