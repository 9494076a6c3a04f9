"""Contact reports (xpbd_world_set_contact_report and the counts / downloads) on the GPU: the pair records and points of the
last substep equal the CPU oracle's SAT at the post-integrate poses bit for bit, the substep counts equal the oracle's
touching sets substep by substep, the events are the set differences of consecutive frames in the documented order, and
reporting changes no bit of the simulation."""
import ctypes as C

import numpy as np
import pytest

import contact_report_model as rm
import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, chain_joints, line_scene, pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body


def cluster(kind, n, seed, spread):
    """test_gpu_pairs.py's cloud of overlapping bodies (a negative spread adds three far bodies: the hashed grid)."""
    rng = np.random.default_rng(seed)
    bodies, sid = capi.scene_generate(kind, seed, n)
    bodies[:, 31:34] = rng.uniform(-abs(spread), abs(spread), (n, 3))
    if spread < 0:
        bodies[[3, 700, 1499], 31:34] = [[4.0e6, 0.0, 0.0], [4.0e6, 0.4, 0.1], [-2.5e6, 7.0e5, 1.0e6]]
    return bodies, sid


def world(kind, bodies, sid, narrowphase=capi.NARROWPHASE_SAT, report=True):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(kind))
    w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    if report:
        w.set_contact_report(True)
    return w


def pair_list(w):
    """The current frame's pair list, from the neighbour lists of its broadphase (no new broadphase)."""
    n_pairs = w.contact_stats()[0]
    off = np.zeros(w.n + 1, dtype=np.uint32)
    nb = np.zeros(max(2 * n_pairs, 1), dtype=np.uint32)
    assert capi.hip_lib().xpbd_world_download_neighbours(w._h, capi._u32(off), capi._u32(nb), nb.size) == capi.OK
    return rm.upper_pairs(off, nb[:off[-1]])


def same_bytes(a, b):
    """Bit-for-bit equality of two record arrays."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def keys_of(pairs):
    return [(int(a), int(b)) for a, b in zip(pairs["body_a"], pairs["body_b"])]


def assert_sorted_and_consistent(pairs, points):
    keys = keys_of(pairs)
    assert all(a < b for a, b in keys) and keys == sorted(set(keys))
    assert np.all(pairs["substeps"] >= 1) and np.all(pairs["reserved"] == 0)
    assert np.array_equal(pairs["first_point"], np.concatenate([[0], np.cumsum(pairs["n_points"])[:-1]]).astype(np.uint32)
                          if len(pairs) else pairs["first_point"])
    assert points is None or len(points) == int(pairs["n_points"].sum())


# ---- 1. the records and points equal the oracle's SAT, the substep counts its touching sets -------------------------------
@pytest.mark.parametrize("kind,n,spread,substeps", [(capi.SCENE_BOXES, 3000, 12.0, 4), (capi.SCENE_MIXED, 300, 0.5, 3),
                                                    (capi.SCENE_MIXED, 1500, -6.0, 3), (capi.SCENE_BOXES, 20000, 32.0, 2)])
def test_report_equals_the_oracle_sat_at_the_post_integrate_poses(kind, n, spread, substeps):
    """(the 300-body clump: one lane per body in the pair solve's neighbour walk; the far bodies: the hashed grid; 20 000
    boxes: above the small-world limit, eight lanes per pair in the SAT)"""
    bodies, sid = cluster(kind, n, 5, spread)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    h = DT / substeps
    with world(kind, bodies, sid) as w:
        w.step(DT, substeps)                     # a frame of settling first: the report then covers a warm frame
        w.contacts_begin(DT)
        pairs = pair_list(w)
        if n > SMALL_WORLD:
            assert len(pairs) >= 32768
        counts = {}
        for k in range(substeps):
            before = w.download()
            frames = rm.p1_frames(before, h)
            touching = rm.manifolds(frames, sid, polys, pairs)
            for key in touching:
                counts[key] = counts.get(key, 0) + 1
            w.contacts_substep(h)
        got, points = w.pair_contacts()
        n_pairs, n_points, _, _ = w.contact_report_counts()
    assert_sorted_and_consistent(got, points)
    assert keys_of(got) == sorted(counts)
    assert [int(s) for s in got["substeps"]] == [counts[k] for k in sorted(counts)]
    assert len(touching) > 50 and n_pairs == len(got) and n_points == len(points)
    features = set()
    for r in got:
        key = (int(r["body_a"]), int(r["body_b"]))
        if key not in touching:
            assert r["n_points"] == 0 and r["feature"] == 0 and r["depth"] == 0.0 and not r["normal"].any()
            continue
        feature, npts, normal, depth, ref, inc = rm.record(frames, sid, polys, key[0], key[1], touching[key])
        features.add(feature)
        assert (int(r["feature"]), int(r["n_points"])) == (feature, npts), key
        assert bits_equal(r["normal"], normal) and bits_equal(np.array([r["depth"]]), np.array([depth])), key
        p = points[r["first_point"]:r["first_point"] + npts]
        assert bits_equal(p["p_ref"], ref) and bits_equal(p["p_inc"], inc), key
    assert capi.FEATURE_FACE_A in features


# ---- 2. GJK + EPA: the report agrees with the pipeline's own statistics -----------------------------------------------------
def test_gjk_epa_report_equals_the_penetrating_pairs_and_the_statistics():
    kind, substeps = capi.SCENE_MIXED, 4
    bodies, sid = cluster(kind, 400, 9, 2.0)
    h = DT / substeps
    polys = ob.polytopes_array(POLY_NAMES[kind])
    with world(kind, bodies, sid, capi.NARROWPHASE_GJK_EPA) as w:
        w.contacts_begin(DT)
        pairs = pair_list(w)
        w.contact_stats()
        first = None
        per_substep = []
        for k in range(substeps):
            if k == 0:                           # nothing is warm-started yet: the plain query decides
                frames = rm.p1_frames(w.download(), h)
                first = sorted((i, j) for i, j in pairs
                               if ob.gjk_epa(frames[i], frames[j], polys[int(sid[i])], polys[int(sid[j])]).status == capi.GJK_PENETRATING)
            w.contacts_substep(h)
            got, points = w.pair_contacts()
            st = w.contact_stats()
            last = got[got["n_points"] > 0]
            assert (len(last), int(last["n_points"].sum())) == (st[1], st[2])
            assert len(points) == st[2]
            per_substep.append(st[1])
            if k == 0:
                assert keys_of(got) == first and np.all(got["n_points"] >= 1)
                assert np.all(got["feature"] <= capi.FEATURE_EDGES)
        assert int(got["substeps"].sum()) == sum(per_substep) and len(first) > 20
        assert_sorted_and_consistent(got, points)


# ---- 3. events ------------------------------------------------------------------------------------------------------------
def test_events_are_the_set_differences_of_consecutive_frames():
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = pile(capi, kind, 400, 3, 4.0, 8.0)
    with world(kind, bodies, sid) as w:
        prev, seen_end, most, history = [], 0, 0, {}
        for frame in range(30):
            if frame == 12:
                index = w.history_push()
            w.step(DT, 8)
            got, points = w.pair_contacts()
            cur = keys_of(got)
            ev = w.contact_events()
            want = rm.events(prev, cur)
            assert [tuple(int(v) for v in e) for e in ev] == want, frame
            c = w.contact_report_counts()
            assert c == (len(got), len(points), sum(1 for e in want if e[2] == capi.CONTACT_BEGIN),
                         sum(1 for e in want if e[2] == capi.CONTACT_END))
            seen_end += c[3]
            most = max(most, len(cur))
            history[frame] = (got, points)
            prev = cur
        assert seen_end > 0 and most > 100
        # restoring the state before frame 12 and stepping: frame 12's pairs and points again, all BEGIN
        w.history_restore(index)
        with pytest.raises(capi.XpbdError):
            w.contact_report_counts()
        w.step(DT, 8)
        got, points = w.pair_contacts()
        assert same_bytes(got, history[12][0]) and same_bytes(points, history[12][1])
        ev = w.contact_events()
        assert np.all(ev["kind"] == capi.CONTACT_BEGIN) and keys_of(ev) == keys_of(got)
        # after enabling, everything is BEGIN too
        w.set_contact_report(True)
        with pytest.raises(capi.XpbdError):
            w.contact_events()
        w.step(DT, 8)
        ev = w.contact_events()
        assert np.all(ev["kind"] == capi.CONTACT_BEGIN) and keys_of(ev) == keys_of(w.pair_contacts()[0])
        # a step in another mode: no report, then S_prev is empty
        w.set_mode(capi.MODE_PER_SUBSTEP)
        w.step(DT, 8)
        with pytest.raises(capi.XpbdError):
            w.pair_contacts()
        w.set_mode(capi.MODE_CONTACTS)
        w.step(DT, 8)
        assert np.all(w.contact_events()["kind"] == capi.CONTACT_BEGIN)
        # an upload: no report, then S_prev is empty.  Frame 12 again, its end state uploaded anew, then frame 13: its pairs, all
        # BEGIN (without the upload its events were a difference against frame 12's pairs)
        w.history_restore(index)
        w.step(DT, 8)
        state = w.download()
        w.upload(state, sid)
        with pytest.raises(capi.XpbdError):
            w.contact_report_counts()
        w.step(DT, 8)
        got = w.pair_contacts()[0]
        ev = w.contact_events()
        assert same_bytes(got, history[13][0])
        assert len(rm.events(keys_of(history[12][0]), keys_of(got))) < len(got)
        assert len(got) > 0 and np.all(ev["kind"] == capi.CONTACT_BEGIN) and keys_of(ev) == keys_of(got)


def test_split_api_capacities_and_argument_errors():
    kind = capi.SCENE_BOXES
    bodies, sid = cluster(kind, 600, 4, 5.0)
    L = capi.hip_lib()
    with world(kind, bodies, sid, report=False) as w:
        n = C.c_uint32(0)
        out = (C.c_uint32 * 4)()
        assert L.xpbd_world_contact_report_counts(w._h, out) == capi.E_INVALID     # reporting off
        assert L.xpbd_world_set_contact_report(w._h, 2) == capi.E_INVALID
        w.set_contact_report(True)
        assert L.xpbd_world_contact_report_counts(w._h, out) == capi.E_INVALID     # nothing run yet
        w.step(DT, 4)
        w.contacts_begin(DT)
        assert L.xpbd_world_contact_report_counts(w._h, out) == capi.E_INVALID     # a frame without substeps
        w.contacts_substep(DT / 4)
        w.contacts_substep(DT / 4)
        pairs, points = w.pair_contacts()
        assert len(pairs) > 10
        small = np.zeros(3, dtype=capi.PAIR_CONTACT_DTYPE)
        m = C.c_uint32(0)
        assert L.xpbd_world_download_pair_contacts(w._h, small.ctypes.data, 3, None, 0, C.byref(n), C.byref(m)) == capi.E_CAPACITY
        assert (n.value, m.value) == (len(pairs), len(points)) and same_bytes(small, pairs[:3])
        few = np.zeros(2, dtype=capi.CONTACT_POINT_DTYPE)
        assert L.xpbd_world_download_pair_contacts(w._h, None, 0, few.ctypes.data, 2, C.byref(n), C.byref(m)) == capi.E_CAPACITY
        assert same_bytes(few, points[:2])
        assert L.xpbd_world_download_pair_contacts(w._h, None, 5, None, 0, C.byref(n), C.byref(m)) == capi.E_INVALID
        assert L.xpbd_world_download_contact_events(w._h, None, 0, C.byref(n)) == (capi.E_CAPACITY if n.value else capi.OK)
        events = w.contact_events()
        assert len(events) > 3
        short = np.zeros(3, dtype=capi.CONTACT_EVENT_DTYPE)
        assert L.xpbd_world_download_contact_events(w._h, short.ctypes.data, 3, C.byref(n)) == capi.E_CAPACITY
        assert n.value == len(events) and same_bytes(short, events[:3])
        assert L.xpbd_world_download_contact_events(w._h, None, 1, C.byref(n)) == capi.E_INVALID
        assert L.xpbd_world_download_contact_events(w._h, None, 0, None) == capi.E_INVALID
        # a third substep: the report follows it
        w.contacts_substep(DT / 4)
        again, _ = w.pair_contacts()
        assert np.all(again["substeps"] >= 1) and int(again["substeps"].max()) <= 3
        w.set_contact_report(False)
        assert L.xpbd_world_contact_report_counts(w._h, out) == capi.E_INVALID


# ---- 5. sharded == single ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_sharded_world_reports_equal_the_single_world(n_ranks):
    """2 and 4 in-process shards on one device, re-planned automatically with a small halo margin (re-plans, migrations and
    undone frames happen): every frame's pairs, points and events equal the single world's bit for bit."""
    kind, n, substeps, frames = capi.SCENE_BOXES_DROP, 96, 6, 30
    rng = np.random.default_rng(n_ranks)
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 25:28] = rng.normal(scale=6.0, size=(n, 3))             # spinning: neighbours bump
    bodies[:, 22] += 1.5                                              # and the line drifts across the cuts: owners change
    want = []
    with world(kind, bodies, sid) as w:
        for _ in range(frames):
            w.step(DT, substeps)
            want.append((*w.pair_contacts(), w.contact_events()))
        one = w.download()
    touching, migrated, plans = 0, 0, 0
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n)
        with pytest.raises(capi.XpbdError):
            mw.contact_report_counts()                                 # reporting off
        mw.set_contact_report(True)
        with pytest.raises(capi.XpbdError):
            mw.contact_events()                                        # nothing stepped yet
        for f in range(frames):
            mw.step(DT, substeps)
            pairs, points = mw.pair_contacts()
            events = mw.contact_events()
            assert same_bytes(pairs, want[f][0]) and same_bytes(points, want[f][1]) and same_bytes(events, want[f][2]), f
            assert mw.contact_report_counts() == (len(pairs), len(points), int((events["kind"] == 0).sum()), int((events["kind"] == 1).sum()))
            touching += len(pairs)
            st = mw.plan_stats()
            if st["plans"] != plans:
                migrated += st["migrated"]
                plans = st["plans"]
        got = mw.download()
        stats = mw.plan_stats()
        # an upload empties S_prev
        mw.upload(got, sid, 0, n)
        with pytest.raises(capi.XpbdError):
            mw.pair_contacts()
        mw.step(DT, substeps)
        assert np.all(mw.contact_events()["kind"] == capi.CONTACT_BEGIN)
    assert bits_equal(got, one) and touching > 100
    assert stats["plans"] > 1 and migrated > 0


# ---- 4. reporting changes no bit --------------------------------------------------------------------------------------------
def limited_chain(n):
    """test_gpu_collision_filter.py's chain: a hinge with a hinge limit and a ball joint with a swing limit among distance joints."""
    joints = chain_joints(capi, n)
    joints["axis_a"], joints["axis_b"] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    joints["kind"][1] = capi.JOINT_HINGE
    lims = np.zeros(2, dtype=capi.JOINT_LIMIT_DTYPE)
    lims["joint"], lims["kind"], lims["lower"], lims["upper"] = [1, 0], [capi.LIMIT_HINGE, capi.LIMIT_SWING], [-0.3, 0.0], [0.3, 0.2]
    lims["ref_a"], lims["ref_b"] = [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]
    return joints, lims


@pytest.mark.parametrize("narrowphase,n", [(capi.NARROWPHASE_SAT, 3000), (capi.NARROWPHASE_GJK_EPA, 1200),
                                           (capi.NARROWPHASE_SAT, 20000)])
def test_reporting_changes_no_bit(narrowphase, n):
    kind = capi.SCENE_MIXED_DROP
    bodies, sid = pile(capi, kind, n, 7, np.sqrt(n) * 0.35, 8.0)
    joints, lims = limited_chain(40)
    rng = np.random.default_rng(2)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1 << rng.integers(0, 3, n), rng.integers(1, 8, n)
    results = []
    for report in (False, True):
        with world(kind, bodies, sid, narrowphase, report=report) as w:
            w.set_joints(joints)
            w.set_joint_limits(lims)
            w.set_collision_filters(filters)
            stats, masks, reported = [], [], 0
            for _ in range(30):
                w.step(DT, 6)
                stats.append(w.contact_stats())
                masks.append(w.contacts())
                if report:
                    reported += len(w.pair_contacts()[0]) + len(w.contact_events())
            results.append((w.download(), stats, masks))
    assert bits_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]
    assert all(np.array_equal(a, b) for a, b in zip(results[0][2], results[1][2]))
    assert reported > 0


def test_a_fully_filtered_pile_reports_nothing():
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = pile(capi, kind, 300, 5, 3.0, 6.0)
    filters = np.zeros(300, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1, 2
    with world(kind, bodies, sid) as w:
        w.set_collision_filters(filters)
        for _ in range(10):
            w.step(DT, 4)
            assert w.contact_report_counts() == (0, 0, 0, 0)


# ---- 6. full size ----------------------------------------------------------------------------------------------------------
def test_full_size_pile_totals_equal_the_statistics():
    bodies, sid = capi.scene_pile(capi.SCENE_BOXES, 0, 262144, 1.8, 4)   # bench.py's boxes pile
    substeps = 20
    with world(capi.SCENE_BOXES, bodies, sid) as w:
        for _ in range(120):                     # fallen and landed
            w.step(DT, substeps)
        w.contacts_begin(DT)
        w.contact_stats()
        per = []
        for _ in range(substeps):
            w.contacts_substep(DT / substeps)
            per.append(w.contact_stats())
        got, points = w.pair_contacts()
    keys = got["body_a"].astype(np.uint64) << np.uint64(32) | got["body_b"].astype(np.uint64)
    assert np.all(np.diff(keys) > 0)
    last = got[got["n_points"] > 0]
    assert (len(last), int(last["n_points"].sum())) == per[-1][1:]
    assert int(got["substeps"].sum()) == sum(p[1] for p in per) and len(points) == per[-1][2]
    assert per[-1][1] > 100000
