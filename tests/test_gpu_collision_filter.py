"""Collision filters (xpbd_world_set_collision_filters, xpbd_multi_world_set_collision_filters, the masked ray casts) on the
GPU: the filtered broadphase equals the oracle's lists minus what the model (tests/collision_filter_model.py) filters out;
filters that filter nothing change no bit; filtering everything gives the reference path; two piles in disjoint groups step
as if each were alone; jointed pairs drop out; a sharded world equals the single one; masked ray casts equal plain casts
on the admitted bodies; bad arguments leave the previous filters in place.  Last, for every body-indexed setting (joints with
limits, filters, materials, restitution): an upload of the same bodies drops it, and a planned sharded world keeps it through
re-plans that move bodies between owners."""
import numpy as np
import pytest

import collision_filter_model as fm
import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, chain_joints, line_scene, pile

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
ALL = 0xFFFFFFFF
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
X, Y, Z = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]


def filters_of(groups, masks):
    f = np.zeros(len(groups), dtype=capi.COLLISION_FILTER_DTYPE)
    f["group"], f["mask"] = groups, masks
    return f


def random_filters(rng, n, layers=4):
    return filters_of(1 << rng.integers(0, layers, n), rng.integers(0, 1 << layers, n))


def cluster(kind, n, seed, spread):
    """test_gpu_pairs.py's cloud of overlapping bodies."""
    rng = np.random.default_rng(seed)
    bodies, sid = capi.scene_generate(kind, seed, n)
    bodies[:, 31:34] = rng.uniform(-spread, spread, (n, 3))
    return bodies, sid


def joints_between(pairs):
    j = np.zeros(len(pairs), dtype=capi.JOINT_DTYPE)
    if len(pairs):
        j["body_a"], j["body_b"] = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
    j["anchor_a"], j["anchor_b"] = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]
    j["distance"] = 1.0
    return j


def world(kind, bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT):
    w = capi.World(mode=mode)
    w.set_polytopes(capi.scene_polytopes(kind))
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


def run(kind, bodies, sid, frames, substeps, joints=None, filters=None, flags=0, set_filters=True, narrowphase=capi.NARROWPHASE_SAT,
        mode=capi.MODE_CONTACTS, lims=None):
    with world(kind, bodies, sid, mode, narrowphase) as w:
        if joints is not None:
            w.set_joints(joints)
        if lims is not None:
            w.set_joint_limits(lims)
        if set_filters:
            w.set_collision_filters(filters, flags)
        for _ in range(frames):
            w.step(DT, substeps)
        return w.download()


# ---- 1. the filtered broadphase is exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,spread", [(capi.SCENE_BOXES, 3000, 12.0), (capi.SCENE_MIXED, 300, 0.5),
                                           (capi.SCENE_MIXED, 1500, -6.0)])
def test_filtered_broadphase_equals_oracle_minus_model(kind, n, spread):
    """Dense grid, the 300-body clump (lists beyond the LDS stage: the one-lane path), and the hashed grid (three bodies
    millions of metres away), as test_gpu_pairs.py::test_broadphase_matches_brute_force; random groups and masks, with
    and without XPBD_FILTER_JOINTED on random joints (half of them between neighbours)."""
    rng = np.random.default_rng(n)
    bodies, sid = cluster(kind, n, 5, abs(spread))
    if spread < 0:
        bodies[[3, 700, 1499], 31:34] = [[4.0e6, 0.0, 0.0], [4.0e6, 0.4, 0.1], [-2.5e6, 7.0e5, 1.0e6]]
    bodies[::7, 22:25] *= 30.0
    want_off, want_nb = ob.broadphase(bodies, sid, ob.polytopes_array(POLY_NAMES[kind]), DT, 0.05)
    near = [(i, int(want_nb[want_off[i]])) for i in rng.choice(n, 60, replace=False) if want_off[i + 1] > want_off[i]]
    far = [(int(a), int(b)) for a, b in rng.integers(0, n, (60, 2)) if a != b]
    joints = joints_between(near + far)
    filters = random_filters(rng, n, layers=2 if spread == 0.5 else 4)
    with world(kind, bodies, sid) as w:
        w.set_contact_pad(0.05)
        w.set_joints(joints)
        for flags in (0, capi.FILTER_JOINTED):
            w.set_collision_filters(filters, flags)
            off, nb = w.neighbours(DT)
            m_off, m_nb = fm.filter_lists(want_off, want_nb, filters, joints, flags == capi.FILTER_JOINTED)
            assert np.array_equal(off, m_off) and np.array_equal(nb, m_nb)
            assert 0 < len(nb) < len(want_nb)
            if spread == 0.5:
                assert np.diff(off).max() > 128                  # the one-lane path is taken
        w.set_collision_filters(None, capi.FILTER_JOINTED)      # joints only
        off, nb = w.neighbours(DT)
        m_off, m_nb = fm.filter_lists(want_off, want_nb, None, joints, True)
        assert np.array_equal(off, m_off) and np.array_equal(nb, m_nb)
        assert len(nb) < len(want_nb)


# ---- 2. filters that filter nothing change no bit -----------------------------------------------------------------------
def limited_chain(n):
    joints = chain_joints(capi, n)
    joints["axis_a"], joints["axis_b"] = Z, Z
    joints["kind"][1] = capi.JOINT_HINGE
    lims = np.zeros(2, dtype=capi.JOINT_LIMIT_DTYPE)
    lims["joint"], lims["kind"], lims["lower"], lims["upper"] = [1, 0], [capi.LIMIT_HINGE, capi.LIMIT_SWING], [-0.3, 0.0], [0.3, 0.2]
    lims["ref_a"], lims["ref_b"] = X, X
    return joints, lims


@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
@pytest.mark.parametrize("n,width", [(160, 4.0), (SMALL_WORLD + 200, 140.0)])
def test_all_ones_filters_change_no_bit(narrowphase, n, width):
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = pile(capi, kind, n, 6, width, 6.0)
    joints, lims = limited_chain(n)
    ones = filters_of(np.full(n, ALL, dtype=np.uint32), np.full(n, ALL, dtype=np.uint32))
    plain = run(kind, bodies, sid, 30, 10, joints, set_filters=False, narrowphase=narrowphase, lims=lims)
    got = run(kind, bodies, sid, 30, 10, joints, ones, 0, narrowphase=narrowphase, lims=lims)
    cleared = run(kind, bodies, sid, 30, 10, joints, None, 0, narrowphase=narrowphase, lims=lims)
    assert not np.isnan(plain).any()
    assert bits_equal(got, plain) and bits_equal(cleared, plain)


# ---- 3. filtering everything gives the reference path -------------------------------------------------------------------
def test_everything_filtered_equals_the_reference_path():
    kind, n = capi.SCENE_BOXES_DROP, 400
    bodies, sid = pile(capi, kind, n, 2, 3.0, 4.0)                   # interpenetrating
    none = filters_of(np.ones(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    with world(kind, bodies, sid) as w:
        assert len(w.neighbours(DT)[1]) > n
        w.set_collision_filters(none)
        off, nb = w.neighbours(DT)
        assert len(nb) == 0 and not off.any()
        for _ in range(20):
            w.step(DT, 20)
        assert w.contact_stats()[0] == 0
        got = w.download()
    ref = run(kind, bodies, sid, 20, 20, set_filters=False, mode=capi.MODE_PER_SUBSTEP)
    assert bits_equal(got, ref)


# ---- 4. superposition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrowphase", [capi.NARROWPHASE_SAT, capi.NARROWPHASE_GJK_EPA])
def test_two_piles_in_disjoint_groups_step_as_if_alone(narrowphase):
    """Two interpenetrating piles over the same ground, interleaved by index (A at even, B at odd slots), A in group 1 and
    B in group 2, each with its own chain of joints: every body ends bit for bit where its pile alone puts it."""
    kind, n = capi.SCENE_BOXES_DROP, 200
    a, sid_a = pile(capi, kind, n, 3, 4.0, 5.0)
    b, sid_b = pile(capi, kind, n, 4, 4.0, 5.0)
    ja, jb = chain_joints(capi, n), chain_joints(capi, n, every=2)
    both = np.empty((2 * n, a.shape[1]))
    both[0::2], both[1::2] = a, b
    sid = np.empty(2 * n, dtype=np.uint32)
    sid[0::2], sid[1::2] = sid_a, sid_b
    jab = np.concatenate([ja, jb])
    jab["body_a"][: len(ja)] *= 2
    jab["body_b"][: len(ja)] *= 2
    jab["body_a"][len(ja):] = 2 * jab["body_a"][len(ja):] + 1
    jab["body_b"][len(ja):] = 2 * jab["body_b"][len(ja):] + 1
    groups = np.tile(np.array([1, 2], dtype=np.uint32), n)
    frames, substeps = 20, 10
    alone_a = run(kind, a, sid_a, frames, substeps, ja, set_filters=False, narrowphase=narrowphase)
    alone_b = run(kind, b, sid_b, frames, substeps, jb, set_filters=False, narrowphase=narrowphase)
    with world(kind, both, sid, narrowphase=narrowphase) as w:
        w.set_joints(jab)
        off, nb = w.neighbours(DT)
        cross = sum(((nb[off[i]:off[i + 1]] % 2) != (i % 2)).sum() for i in range(2 * n))
        assert cross > 0                                            # the piles overlap
        w.set_collision_filters(filters_of(groups, groups))
        for _ in range(frames):
            w.step(DT, substeps)
        got = w.download()
    assert not np.isnan(got).any()
    assert bits_equal(got[0::2], alone_a)
    assert bits_equal(got[1::2], alone_b)


# ---- 5. jointed pairs -------------------------------------------------------------------------------------------------
def straight_chain(n, pitch):
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, n)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 22:28] = 0.0
    bodies[:, 31] = np.arange(n) * pitch
    bodies[:, 32:34] = 0.0
    return bodies, sid


def hinges(n, pitch):
    """Hinges about y halfway between consecutive links (unit cubes, local [0, 1]^3)."""
    j = np.zeros(n - 1, dtype=capi.JOINT_DTYPE)
    j["body_a"], j["body_b"] = np.arange(n - 1), np.arange(1, n)
    j["anchor_a"], j["anchor_b"] = [pitch / 2 + 0.5, 0.5, 0.5], [0.5 - pitch / 2, 0.5, 0.5]
    j["axis_a"] = j["axis_b"] = Y
    j["kind"] = capi.JOINT_HINGE
    return j


def test_jointed_links_that_overlap_at_the_hinges_do_not_touch():
    n, pitch = 12, 0.9                                               # consecutive links overlap by 0.1 m
    bodies, sid = straight_chain(n, pitch)
    joints = hinges(n, pitch)
    for flags, touching in ((0, True), (capi.FILTER_JOINTED, False)):
        with world(capi.SCENE_BOXES, bodies, sid) as w:
            w.set_joints(joints)
            w.set_collision_filters(None, flags)
            off, nb = w.neighbours(DT)
            linked = [(i, i + 1) for i in range(n - 1)]
            present = [int(i + 1) in nb[off[i]:off[i + 1]].tolist() for i, _ in linked]
            assert all(present) if touching else not any(present)
            for _ in range(3):
                w.step(DT, 20)
            assert (w.contact_stats()[1] > 0) == touching


def test_jointed_flag_equals_alternating_groups_on_a_chain():
    n, pitch = 16, 1.05
    bodies, sid = straight_chain(n, pitch)
    joints = hinges(n, pitch)
    with world(capi.SCENE_BOXES, bodies, sid) as w:
        off, nb = w.neighbours(DT)
    want = [sorted({i - 1, i + 1} & set(range(n))) for i in range(n)]
    assert [nb[off[i]:off[i + 1]].tolist() for i in range(n)] == want     # only consecutive links are neighbours
    alt = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)
    out = []
    for filters, flags in ((None, capi.FILTER_JOINTED), (filters_of(alt, alt), 0), (None, 0)):
        with world(capi.SCENE_BOXES, bodies, sid) as w:
            w.set_joints(joints)
            w.set_collision_filters(filters, flags)
            for _ in range(30):
                w.step(DT, 20)
            out.append((w.download(), w.contact_stats()[0]))
    (by_flag, pairs_flag), (by_groups, pairs_groups), (_, pairs_plain) = out
    assert not np.isnan(by_flag).any()
    assert bits_equal(by_flag, by_groups)
    assert pairs_flag == pairs_groups == 0 and pairs_plain == n - 1


# ---- 6. sharded == single -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_sharded_world_with_filters_equals_single(n_ranks):
    kind, n, substeps, frames = capi.SCENE_BOXES_DROP, 96, 6, 30
    rng = np.random.default_rng(n_ranks)
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 25:28] = rng.normal(scale=6.0, size=(n, 3))             # spinning: neighbours bump
    bodies[:, 22] += 1.5                                              # and the line drifts across the cuts: owners change
    joints = chain_joints(capi, n, every=1, distance=0.0, limit=n // 2)
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    filters = random_filters(rng, n, layers=2)
    one = run(kind, bodies, sid, frames, substeps, joints, filters, capi.FILTER_JOINTED)
    assert not bits_equal(one, run(kind, bodies, sid, frames, substeps, joints, set_filters=False))
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        mw.set_collision_filters(filters, capi.FILTER_JOINTED)
        owner = mw.owners()
        migrated = 0
        for f in range(frames):
            mw.step(DT, substeps)
            if f % 6 == 5:
                mw.replan()
                migrated += mw.plan_stats()["migrated"]
        got = mw.download()
        stats = mw.plan_stats()
    assert (owner[joints["body_a"]] != owner[joints["body_b"]]).any()
    assert stats["plans"] > 1 and migrated > 0
    assert not np.isnan(one).any() and bits_equal(got, one)


# ---- 7. masked ray casts ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def down_rays(rng, count, width, ignore=None):
    o = np.column_stack([rng.uniform(-0.5, width + 0.5, (count, 2)), np.full(count, 30.0)])
    d = np.column_stack([rng.normal(scale=0.05, size=(count, 2)), -np.ones(count)])
    return capi.rays(o, d, 100.0, ignore)


@pytest.mark.parametrize("flags", [0, capi.RAYCAST_BRUTE_FORCE])
def test_masked_raycast_equals_plain_cast_on_the_admitted_bodies(flags):
    kind, n, width = capi.SCENE_MIXED_DROP, 3000, 12.0
    rng = np.random.default_rng(9)
    bodies, sid = pile(capi, kind, n, 1, width, 8.0)
    filters = random_filters(rng, n, layers=3)
    filters["group"][::11] = 0                                       # group 0: only the plain cast sees these
    rays = down_rays(rng, 600, width)
    with world(kind, bodies, sid, mode=capi.MODE_FUSED) as w:
        plain = w.raycast(rays, flags)
        assert same_bits(w.raycast(rays, flags, mask=ALL), plain)     # no filters: mask ~0 is the plain call
        w.set_collision_filters(filters)
        assert same_bits(w.raycast(rays, flags), plain)              # the plain call hits every body, group 0 included
        assert np.isin(np.flatnonzero(filters["group"] == 0), plain["body"]).any()
        for mask in (1, 6, 0):
            keep = fm.admitted(filters, n, mask)
            ids = np.flatnonzero(keep).astype(np.uint32)
            r = rays.copy()
            hit_ids = plain["body"][plain["body"] != capi.NO_HIT]
            r["ignore_body"][::5] = hit_ids[: len(r[::5])] if len(hit_ids) else capi.NO_HIT
            got = w.raycast(r, flags, mask=mask)
            sub_r = r.copy()                                        # ignore_body in the numbering of the admitted bodies
            remap = np.full(n, capi.NO_HIT, dtype=np.uint32)
            remap[ids] = np.arange(len(ids))
            ignored = r["ignore_body"] != capi.NO_HIT
            sub_r["ignore_body"][ignored] = remap[r["ignore_body"][ignored]]
            if len(ids):
                with world(kind, bodies[keep], sid[keep], mode=capi.MODE_FUSED) as sub:
                    want = sub.raycast(sub_r, flags)
                hit = want["body"] != capi.NO_HIT
                want["body"][hit] = ids[want["body"][hit]]
            else:                                                   # nothing admitted: every ray misses
                want = np.zeros(len(r), dtype=capi.RAY_HIT_DTYPE)
                want["body"] = want["face"] = capi.NO_HIT
                want["distance"] = np.inf
            assert same_bits(got, want), mask
            assert mask == 0 or (got["body"] != capi.NO_HIT).sum() > 50


def test_multi_world_masked_raycast_equals_single():
    kind, n, width = capi.SCENE_BOXES_DROP, 800, 10.0
    rng = np.random.default_rng(4)
    bodies, sid = pile(capi, kind, n, 5, width, 4.0)
    filters = random_filters(rng, n, layers=2)
    rays = down_rays(rng, 300, width)
    with world(kind, bodies, sid) as w:
        w.set_collision_filters(filters)
        want = [w.raycast(rays, 0, mask=m) for m in (1, 2, 3)]
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=1.0) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n)
        mw.set_collision_filters(filters)
        got = [mw.raycast(rays, 0, mask=m) for m in (1, 2, 3)]
    for g, wt in zip(got, want):
        assert same_bits(g, wt)
    assert not same_bits(want[0], want[2])


# ---- 8. errors and lifetime ---------------------------------------------------------------------------------------------
def test_bad_filters_are_rejected_and_the_previous_ones_stay():
    kind, n = capi.SCENE_BOXES_DROP, 300
    rng = np.random.default_rng(1)
    bodies, sid = pile(capi, kind, n, 7, 3.0, 3.0)
    filters = random_filters(rng, n)
    L = capi.hip_lib()
    with world(kind, bodies, sid) as w:
        full = w.neighbours(DT)
        w.set_collision_filters(filters)
        kept = w.neighbours(DT)
        assert len(kept[1]) < len(full[1])
        for bad in (filters[:-1], np.concatenate([filters, filters[:1]])):
            with pytest.raises(capi.XpbdError) as e:
                w.set_collision_filters(bad)
            assert e.value.code == capi.E_INVALID
        assert L.xpbd_world_set_collision_filters(w._h, None, n, 0) == capi.E_INVALID
        with pytest.raises(capi.XpbdError):
            w.set_collision_filters(filters_of(np.ones(n, np.uint32), np.ones(n, np.uint32)), 2)
        got = w.neighbours(DT)
        assert np.array_equal(got[0], kept[0]) and np.array_equal(got[1], kept[1])
        # history push / restore leave them alone
        w.history_push()
        w.step(DT, 5)
        w.history_restore(0)
        got = w.neighbours(DT)
        assert np.array_equal(got[0], kept[0]) and np.array_equal(got[1], kept[1])
        # set_joints keeps them, and JOINTED follows the new joints
        off0, nb0 = full
        j1 = joints_between([(i, int(nb0[off0[i]])) for i in range(0, n, 3) if off0[i + 1] > off0[i]])
        j2 = joints_between([(i, int(nb0[off0[i + 1] - 1])) for i in range(1, n, 3) if off0[i + 1] > off0[i]])
        w.set_joints(j1)
        w.set_collision_filters(filters, capi.FILTER_JOINTED)
        for j in (j1, j2):
            w.set_joints(j)
            off, nb = w.neighbours(DT)
            m_off, m_nb = fm.filter_lists(off0, nb0, filters, j, True)
            assert np.array_equal(off, m_off) and np.array_equal(nb, m_nb)
        # upload clears the filters and the flag
        w.upload(bodies, sid)
        got = w.neighbours(DT)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])


def test_multi_world_rejects_bad_filters_and_upload_clears_them():
    kind, n = capi.SCENE_BOXES_DROP, 64
    bodies, sid = line_scene(capi, kind, n, 4, 1.05)
    rng = np.random.default_rng(2)
    filters = random_filters(rng, n, layers=2)
    filtered = run(kind, bodies, sid, 8, 6, None, filters)
    plain = run(kind, bodies, sid, 8, 6, None, set_filters=False)
    assert not bits_equal(filtered, plain)
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=2.0, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n)
        mw.set_collision_filters(filters)
        for bad, flags in ((filters[:-1], 0), (filters, 4)):
            with pytest.raises(capi.XpbdError) as e:
                mw.set_collision_filters(bad, flags)
            assert e.value.code == capi.E_INVALID
        for _ in range(8):
            mw.step(DT, 6)
        assert bits_equal(mw.download(), filtered)
        mw.upload(bodies, sid, 0, n)                                   # clears the filters
        for _ in range(8):
            mw.step(DT, 6)
        assert bits_equal(mw.download(), plain)


# ---- 9. every body-indexed setting goes with the bodies it indexed --------------------------------------------------------
def body_settings(n):
    """name -> what sets it on a World or a MultiWorld (the multi world has the first two only)."""
    rng = np.random.default_rng(5)
    joints, lims = limited_chain(n)
    filters = random_filters(rng, n, layers=2)
    mu = rng.choice([0.0, 0.2, 0.5, 1.0, np.inf], n)
    e = rng.choice([0.0, 0.3, 0.8, 1.0], n)
    return {"filters": lambda w: w.set_collision_filters(filters, capi.FILTER_JOINTED),
            "materials": lambda w: w.set_materials(mu, 0.3),
            "joints with limits": lambda w: (w.set_joints(joints), w.set_joint_limits(lims)),
            "restitution": lambda w: w.set_restitution(e, 0.5, 0.02)}


def stepped(w, frames, substeps):
    for _ in range(frames):
        w.step(DT, substeps)
    return w.download()


@pytest.mark.parametrize("setting", ["joints with limits", "filters", "materials", "restitution"])
def test_upload_of_the_same_bodies_drops_every_body_indexed_setting(setting):
    kind, n, frames, substeps = capi.SCENE_BOXES_DROP, 200, 12, 6
    bodies, sid = pile(capi, kind, n, 7, 4.0, 3.0)
    with world(kind, bodies, sid) as w:
        plain = stepped(w, frames, substeps)                          # a world that never had the setting
    with world(kind, bodies, sid) as w:
        body_settings(n)[setting](w)
        with_setting = stepped(w, frames, substeps)
        w.upload(bodies, sid)
        again = stepped(w, frames, substeps)
    assert not np.isnan(plain).any() and not np.isnan(with_setting).any()
    assert not bits_equal(with_setting, plain)                        # the setting matters in this scene
    assert bits_equal(again, plain)


@pytest.mark.parametrize("setting", ["filters", "materials"])
def test_setting_given_to_a_planned_multi_world_survives_forced_replans_with_migration(setting):
    """The migrating line of test_sharded_world_with_filters_equals_single; the setting arrives after the first plan, so the
    setter hands it to the shards itself, and every later plan hands it over again to the bodies' new owners."""
    kind, n, substeps, before, frames = capi.SCENE_BOXES_DROP, 96, 6, 6, 24
    rng = np.random.default_rng(3)
    bodies, sid = line_scene(capi, kind, n, 11, 1.3)
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    bodies[:, 25:28] = rng.normal(scale=6.0, size=(n, 3))
    bodies[:, 22] += 1.5
    joints = chain_joints(capi, n, every=1, distance=0.0, limit=n // 2)
    joints["anchor_a"], joints["anchor_b"] = [1.15, 0.5, 0.5], [-0.15, 0.5, 0.5]
    apply = body_settings(n)[setting]
    with world(kind, bodies, sid) as w:
        w.set_joints(joints)
        plain = stepped(w, before + frames, substeps)
    with world(kind, bodies, sid) as w:
        w.set_joints(joints)
        stepped(w, before, substeps)
        apply(w)
        one = stepped(w, frames, substeps)
    assert not np.isnan(one).any() and not bits_equal(one, plain)
    with capi.MultiWorld(4, devices=[0] * 4, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n, joints)
        for _ in range(before):
            mw.step(DT, substeps)
        assert mw.plan_stats()["plans"] >= 1
        apply(mw)
        migrated = 0
        for f in range(frames):
            mw.step(DT, substeps)
            if f % 6 == 5:
                mw.replan()
                migrated += mw.plan_stats()["migrated"]
        got = mw.download()
    assert migrated > 0
    assert bits_equal(got, one)
