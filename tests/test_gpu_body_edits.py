"""Body edits (include/xpbd.h, "Body EDITS") on the GPU: forces, impulses and state of resident bodies without re-upload.
The property everything rests on -- a world after an edit steps bit for bit like a fresh world into which the edited
xpbd_rigid array was uploaded -- in every mode and under both narrowphases; the impulse kernel against body_edit_model.py bit
for bit; the settings an upload would drop survive; rejected calls change nothing; the device variants are stream-ordered;
and the sharded world equals the single one, ghosts included, also after a re-plan.  EXTENSION: parity unpinned."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import body_edit_common as bc
import body_edit_model as bm
from body_edit_common import DT, FRAMES, N, STATIC_BODY, SUBSTEPS, scene, stepped, world
from constraint_solver_amd import capi
from halo_common import chain_joints, line_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MIXED, BOXES = capi.SCENE_MIXED_DROP, capi.SCENE_BOXES_DROP
DYN_COLUMNS = [31, 32, 33, 34, 35, 36, 37, 22, 23, 24, 25, 26, 27]      # a row of get_dynamics in xpbd_rigid's doubles
POSE = slice(31, 38)
MODES = [(capi.MODE_FUSED, capi.NARROWPHASE_SAT), (capi.MODE_PER_SUBSTEP, capi.NARROWPHASE_SAT),
         (capi.MODE_CONTACTS, capi.NARROWPHASE_SAT), (capi.MODE_CONTACTS, capi.NARROWPHASE_GJK_EPA)]


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def wrench_edits(w, force, torque):
    """Every form of the call; returns the xpbd_rigid columns they amount to."""
    listed = np.array([129, 0, 64, 63, 17, STATIC_BODY], dtype=np.uint32)
    want_f, want_t = np.zeros((N, 3)), np.zeros((N, 3))
    w.set_external_wrench(None, force=force * 0.5)                       # indices == NULL, force only
    want_f[:] = force * 0.5
    w.set_external_wrench(np.arange(N - 1, -1, -2, dtype=np.uint32), torque=torque[::-2])      # a list, torque only
    want_t[::-2] = torque[::-2]
    w.set_external_wrench(listed, force[listed], -torque[listed])        # both, bodies 0, 63, 64 and 129 among them
    want_f[listed], want_t[listed] = force[listed], -torque[listed]
    w.set_external_wrench(np.zeros(0, dtype=np.uint32), np.zeros((0, 3)), np.zeros((0, 3)))    # n == 0 does nothing
    return want_f, want_t


# ---- 1. a wrench edit equals a re-upload -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [MIXED, BOXES])
@pytest.mark.parametrize("mode,narrowphase", MODES)
def test_wrench_edit_steps_like_a_world_uploaded_with_the_forces(kind, mode, narrowphase):
    bodies, sid = scene(kind)
    force, torque = bc.wrench_values(3)
    with world(kind, bodies, sid, mode, narrowphase) as a:
        want_f, want_t = wrench_edits(a, force, torque)
        edited = a.download()
        got = stepped(a)
    uploaded = bodies.copy()
    uploaded[:, 10:13], uploaded[:, 16:19] = want_f, want_t
    assert same(edited, uploaded)                                        # the edit wrote those two fields and nothing else
    with world(kind, uploaded, sid, mode, narrowphase) as b:
        want = stepped(b)
    assert same(got[0], want[0]) and same(got[1], want[1])
    with world(kind, bodies, sid, mode, narrowphase) as plain:
        assert not same(stepped(plain)[0], want[0])                      # ... and the forces do matter to the run


# ---- 2. impulses equal the model bit for bit -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_child(tmp_path_factory):
    """body_edit_device_child.py, once: the device variants driven from torch tensors on a torch stream."""
    out = tmp_path_factory.mktemp("body_edits") / "device.npz"
    p = subprocess.run([sys.executable, os.path.join(HERE, "body_edit_device_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out))


def test_impulses_equal_the_model_bit_for_bit(device_child):
    bodies, sid = scene(MIXED)
    entries = bc.shuffled(bc.impulse_list(bodies, 11), 12)               # host order shuffled: the stable sort is exercised
    assert set(entries["flags"].tolist()) == {capi.IMPULSE_AT_POINT, capi.IMPULSE_AT_CENTRE}
    assert np.any(np.diff(entries["body"].astype(np.int64)) < 0)
    want = bm.apply_impulses(bodies, entries)
    with world(MIXED, bodies, sid) as w:
        w.apply_impulses(entries)
        got = w.download()
    assert same(got[:, 22:28], want[:, 22:28])
    assert same(got, want)                                               # positions, rotations and the static fields: unchanged bytes
    assert same(got[:, POSE], bodies[:, POSE])
    assert same(got[STATIC_BODY], bodies[STATIC_BODY])                   # inverse_mass == 0: + 0.0
    assert not same(got[64, 22:28], bodies[64, 22:28])
    assert same(device_child["impulses_device"], want)                   # apply_impulses_device with the pre-sorted list
    assert same(device_child["beyond"], want)                            # an entry naming body == body count changes nothing


# ---- 3. impulse then step equals re-upload then step ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,narrowphase", [(MIXED, capi.NARROWPHASE_SAT), (MIXED, capi.NARROWPHASE_GJK_EPA), (BOXES, capi.NARROWPHASE_SAT)])
def test_impulse_edit_steps_like_a_world_uploaded_with_the_velocities(kind, narrowphase):
    bodies, sid = scene(kind)
    entries = bc.shuffled(bc.impulse_list(bodies, 5), 6)
    with world(kind, bodies, sid, narrowphase=narrowphase) as a:
        a.step(DT, SUBSTEPS)                                             # an edit between frames, not only before the first
        before = a.download()
        a.apply_impulses(entries)
        edited = a.download()
        got = stepped(a)
    assert same(edited, bm.apply_impulses(before, entries))
    with world(kind, edited, sid, narrowphase=narrowphase) as b:
        want = stepped(b)
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---- 4. the settings an upload drops survive an edit ----------------------------------------------------------------------------
def settings(w, joints, lims, filters, mu, e):
    w.set_joints(joints)
    w.set_joint_limits(lims)
    w.set_collision_filters(filters, capi.FILTER_JOINTED)
    w.set_materials(mu, 0.6)
    w.set_restitution(e, 0.5, 0.1)
    w.set_contact_report(True)


def keys_of(pairs):
    return set(zip(pairs["body_a"].tolist(), pairs["body_b"].tolist()))


def events_between(prev, cur):
    """BEGINs in key order, then ENDs in key order, as (body_a, body_b, kind)."""
    return [(a, b, capi.CONTACT_BEGIN) for a, b in sorted(cur - prev)] + [(a, b, capi.CONTACT_END) for a, b in sorted(prev - cur)]


def events_of(w):
    ev = w.contact_events()
    return list(zip(ev["body_a"].tolist(), ev["body_b"].tolist(), ev["kind"].tolist()))


def test_settings_history_and_reports_survive_the_edits():
    kind = BOXES
    bodies, sid = scene(kind, seed=6)
    rng = np.random.default_rng(8)
    joints = chain_joints(capi, N)
    joints["axis_a"], joints["axis_b"] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    joints["kind"][1] = capi.JOINT_HINGE
    lims = np.zeros(1, dtype=capi.JOINT_LIMIT_DTYPE)
    lims["joint"], lims["kind"], lims["lower"], lims["upper"] = 1, capi.LIMIT_HINGE, -0.2, 0.3
    lims["ref_a"], lims["ref_b"] = [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]
    filters = np.zeros(N, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1 << rng.integers(0, 2, N), 3
    filters["mask"][::7] = 1
    mu, e = rng.uniform(0.1, 0.9, N), np.full(N, 0.5)
    force, torque = bc.wrench_values(9)
    listed = np.sort(rng.choice(N, 40, replace=False)).astype(np.uint32)
    entries = bc.shuffled(bc.impulse_list(bodies, 13), 14)

    with world(kind, bodies, sid) as a:
        settings(a, joints, lims, filters, mu, e)
        a.step(DT, SUBSTEPS)
        a.step(DT, SUBSTEPS)
        touching_before = keys_of(a.pair_contacts(points=False)[0])
        assert a.history_push() == 0
        pre_edit = a.download()
        a.set_external_wrench(listed, force[listed], torque[listed])
        a.apply_impulses(entries)
        assert a.history_length() == 1
        edited = a.download()
        a.step(DT, SUBSTEPS)
        first_events, first_pairs = events_of(a), a.pair_contacts()
        a.step(DT, SUBSTEPS)
        second_events = events_of(a)
        got = (a.download(), a.contacts())
        assert a.history_length() == 1
        a.history_restore(0)                                             # the entry is still the pre-edit state ...
        restored = a.download()
    assert same(edited[:, 10:13][listed], force[listed]) and same(edited[:, 16:19][listed], torque[listed])
    assert same(restored[:, 10:22], edited[:, 10:22])                    # ... and restoring it does not bring old forces back
    assert same(restored[:, 22:38], pre_edit[:, 22:38]) and not same(restored[:, 22:28], edited[:, 22:28])

    with world(kind, edited, sid) as b:                                  # bodies that carried the forces from the start
        settings(b, joints, lims, filters, mu, e)
        b.step(DT, SUBSTEPS)
        b_first_pairs = b.pair_contacts()
        b.step(DT, SUBSTEPS)
        b_second_events = events_of(b)
        want = (b.download(), b.contacts())
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert touching_before and keys_of(b_first_pairs[0])
    for x, y in zip(first_pairs, b_first_pairs):
        assert same(x, y)
    # S_prev outlives the edit (an upload empties it): the frame after the edit reports against the frame before it
    assert first_events == events_between(touching_before, keys_of(b_first_pairs[0]))
    assert first_events != events_between(set(), keys_of(b_first_pairs[0]))
    assert second_events == b_second_events


# ---- 5. set_dynamics / get_dynamics -------------------------------------------------------------------------------------------
def test_get_dynamics_is_the_thirteen_columns_of_download():
    bodies, sid = scene(MIXED)
    with world(MIXED, bodies, sid) as w:
        w.step(DT, SUBSTEPS)
        state = w.download()
        assert same(w.get_dynamics(), np.ascontiguousarray(state[:, DYN_COLUMNS]))
        idx = np.array([129, 5, 5, 64, 0, 63], dtype=np.uint32)          # get may list a body twice
        assert same(w.get_dynamics(idx), np.ascontiguousarray(state[idx][:, DYN_COLUMNS]))
        assert w.get_dynamics(np.zeros(0, dtype=np.uint32)).shape == (0, 13)
        assert same(w.download(), state)


def test_set_dynamics_teleports_and_steps_like_a_reupload_and_rays_see_the_new_pose():
    bodies, sid = scene(MIXED)
    idx = np.array([129, 0, 64, 63, 17], dtype=np.uint32)
    half = math.sqrt(0.5)
    with world(MIXED, bodies, sid) as a:
        a.step(DT, SUBSTEPS)
        state = a.download()
        rows = np.ascontiguousarray(state[idx][:, DYN_COLUMNS])
        rows[:, 0:3] = [[40.0 + 3.0 * k, -25.0, 2.0 + k] for k in range(len(idx))]       # far from the pile and from each other
        rows[:, 3:7] = [half, 0.0, 0.0, half]
        rows[:, 7:10] = [1.0, -2.0, 3.0]
        rows[:, 10:13] = [0.0, 0.5, 0.0]
        a.set_dynamics(idx, rows)
        edited = a.download()
        want_state = state.copy()
        want_state[idx[:, None], np.array(DYN_COLUMNS)[None, :]] = rows
        assert same(edited, want_state)
        assert same(a.get_dynamics(idx), rows)
        # a ray straight down on the teleported body 129 (nothing else is near x = 40, y = -25)
        centre = edited[129, 31:34] + edited[129, 28:31]
        hit = a.raycast(capi.rays([centre + [0.0, 0.0, 10.0]], [[0.0, 0.0, -1.0]]))[0]
        assert hit["body"] == 129 and 8.0 < hit["distance"] < 10.0
        got = stepped(a)
    with world(MIXED, edited, sid) as b:
        want = stepped(b)
    assert same(got[0], want[0]) and same(got[1], want[1])
    with world(MIXED, bodies, sid) as w:                                 # the whole world in one call, indices == NULL
        w.set_dynamics(None, np.ascontiguousarray(edited[:, DYN_COLUMNS]))
        all_set = w.download()
    assert same(all_set[:, DYN_COLUMNS], edited[:, DYN_COLUMNS]) and same(all_set[:, 0:22], bodies[:, 0:22])


# ---- 6. rejected calls change nothing -----------------------------------------------------------------------------------------
def rejected_calls():
    idx = np.array([3, 129, 64], dtype=np.uint32)
    xyz, rows = np.ones((3, 3)), np.zeros((3, 13))
    rows[:, 3] = 1.0
    imp = capi.impulses([3, 129, 64], [1.0, 0.0, 0.0], point=[0.0, 0.0, 1.0])

    def with_(a, where, value):
        a = a.copy()
        a[where] = value
        return a

    def imp_with(field, value, flags=None):
        e = imp.copy()
        e[field][1] = value
        if flags is not None:
            e["flags"][1] = flags
        return e

    L = capi.hip_lib()
    p = lambda a: None if a is None else a.ctypes.data    # noqa: E731
    wrench = lambda i, n, f, t: ("xpbd_world_set_external_wrench", lambda h: L.xpbd_world_set_external_wrench(h, p(i), n, p(f), p(t)))   # noqa: E731
    impulses = lambda e, n: ("xpbd_world_apply_impulses", lambda h: L.xpbd_world_apply_impulses(h, p(e), n))   # noqa: E731
    set_dyn = lambda i, n, r: ("xpbd_world_set_dynamics", lambda h: L.xpbd_world_set_dynamics(h, p(i), n, p(r)))   # noqa: E731
    get_dyn = lambda i, n, r: ("xpbd_world_get_dynamics", lambda h: L.xpbd_world_get_dynamics(h, p(i), n, p(r)))   # noqa: E731
    return {
        "wrench: NULL force and torque": wrench(idx, 3, None, None),
        "wrench: index == body count": wrench(with_(idx, 1, N), 3, xyz, xyz),
        "wrench: index twice": wrench(with_(idx, 2, 3), 3, xyz, xyz),
        "wrench: NULL indices with n != body count": wrench(None, 3, xyz, xyz),
        "wrench: NaN force": wrench(idx, 3, with_(xyz, (1, 2), np.nan), xyz),
        "wrench: infinite torque": wrench(idx, 3, None, with_(xyz, (2, 0), np.inf)),
        "impulses: NULL list": impulses(None, 3),
        "impulses: body == body count": impulses(imp_with("body", N), 3),
        "impulses: unknown flags": impulses(imp_with("flags", 2), 3),
        "impulses: NaN impulse": impulses(imp_with("impulse", [0.0, np.nan, 0.0]), 3),
        "impulses: infinite point": impulses(imp_with("point", [np.inf, 0.0, 0.0]), 3),
        "impulses: NaN angular impulse": impulses(imp_with("angular_impulse", [0.0, 0.0, np.nan], capi.IMPULSE_AT_CENTRE), 3),
        "set_dynamics: NULL rows": set_dyn(idx, 3, None),
        "set_dynamics: index == body count": set_dyn(with_(idx, 0, N), 3, rows),
        "set_dynamics: index twice": set_dyn(with_(idx, 1, 64), 3, rows),
        "set_dynamics: NULL indices with n != body count": set_dyn(None, 3, rows),
        "set_dynamics: NaN row value": set_dyn(idx, 3, with_(rows, (2, 12), np.nan)),
        "get_dynamics: NULL rows": get_dyn(idx, 3, None),
        "get_dynamics: index == body count": get_dyn(with_(idx, 2, N), 3, rows),
    }


def test_rejected_calls_change_nothing_and_name_themselves():
    bodies, sid = scene(MIXED)
    L = capi.hip_lib()
    with world(MIXED, bodies, sid) as w:
        w.set_external_wrench(None, *bc.wrench_values(1))
        w.step(DT, SUBSTEPS)
        before = w.download()
        for case, (name, call) in rejected_calls().items():
            assert call(w._h) == capi.E_INVALID, case
            assert name.encode() in L.xpbd_last_error(), (case, L.xpbd_last_error())
            assert same(w.download(), before), case
        # an impulse at the centre ignores its point, whatever it holds
        w.apply_impulses(capi.impulses([7], [0.0, 0.0, 0.0]))
        e = capi.impulses([7], [0.0, 0.0, 0.0])
        e["point"] = np.nan
        w.apply_impulses(e)
    with capi.World(mode=capi.MODE_CONTACTS) as empty:                   # no resident bodies
        empty.set_polytopes(capi.scene_polytopes(MIXED))
        one = np.zeros(1, dtype=np.uint32)
        for name, rc in (("xpbd_world_set_external_wrench", L.xpbd_world_set_external_wrench(empty._h, one.ctypes.data, 1, np.zeros(3).ctypes.data, None)),
                         ("xpbd_world_apply_impulses", L.xpbd_world_apply_impulses(empty._h, capi.impulses([0], [0.0, 0.0, 0.0]).ctypes.data, 1)),
                         ("xpbd_world_set_dynamics", L.xpbd_world_set_dynamics(empty._h, one.ctypes.data, 1, np.zeros(13).ctypes.data)),
                         ("xpbd_world_get_dynamics", L.xpbd_world_get_dynamics(empty._h, one.ctypes.data, 1, np.zeros(13).ctypes.data))):
            assert rc == capi.E_INVALID, name
        assert L.xpbd_world_apply_impulses(empty._h, None, 0) == capi.OK  # n == 0 is fine on any live world


# ---- 7. the device variant is ordered on the world's stream -------------------------------------------------------------------
def test_device_wrench_from_a_torch_tensor_then_step_without_a_wait_equals_the_host_variant(device_child):
    bodies, sid = scene(MIXED)
    force, torque = bc.wrench_values(21)
    idx = np.array([129, 0, 64, 63, 17, 100], dtype=np.uint32)
    with world(MIXED, bodies, sid) as w:
        w.set_external_wrench(idx, force[idx], torque[idx])
        w.step(DT, SUBSTEPS)
        w.set_external_wrench(None, force=force)
        want = stepped(w, FRAMES - 1)
    assert same(device_child["wrench_bodies"], want[0]) and same(device_child["wrench_contacts"], want[1])


# ---- 8. the sharded world equals the single one ------------------------------------------------------------------------------
def cut_neighbours(bodies, owner, each=3):
    """The bodies next to every cut between two owners along x: boundary bodies, mirrored as ghosts on the other side."""
    order = np.argsort(bodies[:, 31], kind="stable")
    cuts = np.flatnonzero(np.diff(owner[order].astype(np.int64)) != 0)
    return np.unique(np.concatenate([order[max(c - each + 1, 0): c + 1 + each] for c in cuts])).astype(np.uint32)


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_sharded_world_with_edits_equals_the_single_world_also_after_a_replan(n_ranks):
    kind, substeps = MIXED, 8
    bodies, sid = line_scene(capi, kind, N, 4, 1.4)                      # the mixed scene stretched along x
    bodies[:, 33] += 0.6                                                 # (its icosahedra start inside the ground)
    force, torque = bc.wrench_values(17)
    force, torque = force * 0.2, torque * 0.2

    def edits(w, near_cuts):
        """Before the first frame and between frames; owned, boundary (ghosts elsewhere) and interior bodies."""
        w.set_external_wrench(None, force=force)                         # every body: every ghost is edited
        w.set_external_wrench(near_cuts, torque=torque[near_cuts])
        entries = bc.shuffled(bc.impulse_list(bodies, 19), 20)           # every body, runs and both flags
        w.apply_impulses(entries)
        w.step(DT, substeps)
        w.apply_impulses(capi.impulses(near_cuts, [0.3, 0.0, 0.5]))
        w.set_external_wrench(near_cuts[::2], force=-force[near_cuts[::2]], torque=torque[near_cuts[::2]] * 0.5)
        for _ in range(FRAMES - 1):
            w.step(DT, substeps)

    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=1.5, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, N)
        owner, stats = mw.owners(), mw.halo_stats()
        # every shard owns bodies and mirrors some: with all bodies edited, edited bodies are ghosts somewhere
        assert sorted(set(owner.tolist())) == list(range(n_ranks)), "a shard owns nothing"
        assert stats["ghosts"] >= n_ranks and stats["boundary"] > 0, "no ghosts: the edits would not reach a ghost copy"
        near_cuts = cut_neighbours(bodies, owner)
        assert len(set(owner[near_cuts].tolist())) == n_ranks
        edits(mw, near_cuts)
        sharded = mw.download()
        plans = mw.plan_stats()["plans"]
        mw.replan()                                                      # the forces are part of the records that travel
        assert mw.plan_stats()["plans"] == plans + 1
        for _ in range(2):
            mw.step(DT, substeps)
        sharded_later = mw.download()
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies, sid)
        edits(w, near_cuts)
        single = w.download()
        for _ in range(2):
            w.step(DT, substeps)
        single_later = w.download()
    assert not np.isnan(single_later).any()
    assert same(sharded, single)
    assert same(sharded_later, single_later)
    assert not same(single[:, 10:13], bodies[:, 10:13])


def test_multi_world_rejects_bad_edits_and_changes_nothing():
    bodies, sid = line_scene(capi, MIXED, N, 4, 1.4)
    bodies[:, 33] += 0.6
    L = capi.hip_lib()
    idx = np.array([3, N], dtype=np.uint32)
    xyz = np.ones((2, 3))
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=0.75) as mw:
        mw.set_polytopes(capi.scene_polytopes(MIXED))
        assert L.xpbd_multi_world_apply_impulses(mw._h, capi.impulses([0], [1.0, 0.0, 0.0]).ctypes.data, 1) == capi.E_INVALID   # nothing uploaded
        mw.upload(bodies, sid, 0, N)
        before = mw.download()
        assert L.xpbd_multi_world_set_external_wrench(mw._h, idx.ctypes.data, 2, xyz.ctypes.data, None) == capi.E_INVALID
        assert b"xpbd_multi_world_set_external_wrench" in L.xpbd_last_error()
        bad = capi.impulses([3, 4], [1.0, 0.0, 0.0])
        bad["flags"][1] = 6
        assert L.xpbd_multi_world_apply_impulses(mw._h, bad.ctypes.data, 2) == capi.E_INVALID
        assert b"xpbd_multi_world_apply_impulses" in L.xpbd_last_error()
        assert same(mw.download(), before)
