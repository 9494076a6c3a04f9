"""The edge bodies of tests/edge_rigids.py through the C ABI: every path bit for bit against the oracle (contact masks of
every substep included), and the HIP output itself within the extended-precision model's bound (xprec_cases.K), not only
by transitivity.  The exact-height cases are compared with the oracle alone, NaN-ness for NaN results."""
import numpy as np
import pytest

import edge_rigids as er
import oracle_binding as ob
import xprec_cases as xc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

CONFIG_IDS = ["dt%.4g-S%d" % c[:2] for c in xc.CONFIGS]
CONTACTS_CONFIG = 2                                         # 1/60 s, 20 substeps, 6 frames


def assert_oracle_frames(got, t, sel=None):
    sel = np.arange(len(t["labels"])) if sel is None else sel
    for f, (state, masks) in enumerate(got):
        _, want, want_masks, _ = t["frames"][f]
        if masks is not None:
            assert np.array_equal(masks, want_masks[:, sel]), "contact masks differ in frame %d" % f
        assert bits_equal(state, want[sel]), "state differs from the oracle in frame %d" % f


def run_world(t, dt, substeps, mode, block_size=0, sel=None, bodies=None, polytopes=None):
    sel = np.arange(len(t["labels"])) if sel is None else sel
    out = []
    with capi.World(mode=mode, trace_contacts=True, block_size=block_size) as w:
        if polytopes is None:
            w.set_shapes(t["verts"], t["off"])
        else:
            w.set_polytopes(polytopes)
        w.upload(t["start"][sel] if bodies is None else bodies, t["sid"][sel])
        for _ in range(len(t["frames"])):
            w.step(dt, substeps)
            out.append((w.download(), w.contact_masks(substeps)))
        stats = w.contact_stats() if mode == capi.MODE_CONTACTS else None
    return out, stats


@pytest.mark.parametrize("config", range(len(xc.CONFIGS)), ids=CONFIG_IDS)
@pytest.mark.parametrize("mode,block_size", [(capi.MODE_FUSED, 64), (capi.MODE_FUSED, 256), (capi.MODE_PER_SUBSTEP, 64),
                                             (capi.MODE_PER_SUBSTEP, 256)])
def test_pinned_path_on_edge_bodies(config, mode, block_size):
    dt, substeps, _ = xc.CONFIGS[config]
    t = xc.trajectory(config)
    got, _ = run_world(t, dt, substeps, mode, block_size)
    assert_oracle_frames(got, t)
    xc.check_against_model(config, got)


def test_step_one_on_edge_bodies():
    config = 1
    dt, substeps, _ = xc.CONFIGS[config]
    t = xc.trajectory(config)
    _, want, _, _ = t["frames"][0]
    got = np.array([capi.step_one(b, t["verts"][t["off"][s]:t["off"][s + 1]], dt, substeps) for b, s in zip(t["start"], t["sid"])])
    assert bits_equal(got, want)
    frames = [(got, None)] + [(w, None) for (_, w, _, _) in t["frames"][1:]]
    xc.check_against_model(config, frames)


def apart(states, sid, verts, off, keep):
    """The bodies of `keep` whose bounding spheres, swept over every frame of the trajectory `states` (start and frame
    ends), stay 1 m clear of each other's: the contacts pipeline then finds no pair and adds nothing to the ground
    path.  Bodies with the most near misses are dropped first (the force category's fastest fly for tens of metres)."""
    keep = list(keep)
    com = states[0][:, 28:31]
    r = np.array([np.linalg.norm(verts[off[s]:off[s + 1]] - c, axis=1).max() for s, c in zip(sid, com)]) + 0.02
    centre = np.array([b[:, 31:34] + com for b in states])                               # (frames + 1, n, 3)
    reach = r + np.concatenate([np.linalg.norm(np.diff(centre, axis=0), axis=2), np.zeros((1, len(r)))]).max(axis=0)
    while True:
        k = np.array(keep)
        d = np.linalg.norm(centre[:, k, None, :] - centre[:, None, k, :], axis=3).min(axis=0)
        near = d < reach[k, None] + reach[None, k] + 1.0
        np.fill_diagonal(near, False)
        if not near.any():
            return k
        keep.pop(int(near.sum(axis=1).argmax()))


def contacts_bodies():
    t = xc.trajectory(CONTACTS_CONFIG)
    states = [t["start"]] + [want for (_, want, _, _) in t["frames"]]
    sel = apart(states, t["sid"], t["verts"], t["off"], np.nonzero(t["sid"] != er.HULL32)[0])   # HULL32 has no topology
    assert len(set(t["labels"][sel])) == len(er.CATEGORIES) and len(sel) > 0.8 * len(t["labels"])
    return t, sel


def test_contacts_mode_on_edge_bodies_with_per_body_statics():
    """Statics not shared: the contact kernels gather a static record per body."""
    dt, substeps, _ = xc.CONFIGS[CONTACTS_CONFIG]
    t, sel = contacts_bodies()
    got, stats = run_world(t, dt, substeps, capi.MODE_CONTACTS, sel=sel, polytopes=er.polytopes())
    assert stats[0] == 0                                    # no bounding spheres overlap: the ground path alone
    assert_oracle_frames(got, t, sel)
    xc.check_against_model(CONTACTS_CONFIG, got, sel)


@pytest.mark.parametrize("odd_one", [False, True], ids=["shared", "one-ulp-off"])
def test_contacts_mode_on_edge_bodies_with_shared_statics(odd_one):
    """Statics shared per shape bit for bit (the kernels read the per-shape table), and the same with one body one ulp
    off in an off-diagonal inverse inertia entry (the per-body fallback)."""
    dt, substeps, frames = xc.CONFIGS[CONTACTS_CONFIG]
    t, sel = contacts_bodies()
    bodies = er.share_statics(t["start"][sel], t["sid"][sel])
    if odd_one:
        bodies[5, 2] = np.nextafter(bodies[5, 2], np.inf)
    want, want_masks = bodies, []
    for _ in range(frames):
        want, m = ob.step_bodies(want, t["sid"][sel], t["verts"], t["off"], dt, substeps, want_masks=True)
        want_masks.append((want, m))
    got, stats = run_world(t, dt, substeps, capi.MODE_CONTACTS, sel=sel, bodies=bodies, polytopes=er.polytopes())
    assert stats[0] == 0
    for f in range(frames):
        assert np.array_equal(got[f][1], want_masks[f][1]) and bits_equal(got[f][0], want_masks[f][0]), f


def test_two_shard_multi_world_moves_edge_statics_bit_for_bit():
    """Two shards on TRANSPORT_LOCAL; every body drifts 0.2 m per frame along x, across the cut, so re-plans re-pack and
    migrate bodies with non-zero forces, torques and asymmetric inertia.  Equal to the single world and to the oracle.
    Bodies that move 0.4 m or more in a frame are left out: the library undoes such a frame (XPBD_E_HALO)."""
    config = 1
    dt, substeps, _ = xc.CONFIGS[config]
    t = xc.trajectory(config)
    start = t["start"].copy()
    start[:, 22] += 12.0
    frames = 45
    states = [start]
    for _ in range(frames):
        states.append(ob.step_bodies(states[-1], t["sid"], t["verts"], t["off"], dt, substeps)[0])
    step = np.linalg.norm(np.diff(np.array([b[:, 31:34] for b in states]), axis=0), axis=2).max(axis=0)
    slow = np.nonzero((t["sid"] != er.HULL32) & (step < 0.4))[0]      # within halo_margin 0.5 m per frame, as the library needs
    sel = apart(states, t["sid"], t["verts"], t["off"], slow)
    assert {"force", "asym_inertia", "ulp_shared"} <= set(t["labels"][sel])
    assert (np.abs(start[sel, 13:22]).max(axis=1) > 0).sum() >= 10       # forces and torques do move between the shards
    bodies, sid = start[sel], t["sid"][sel]
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=0.5, auto_replan=True) as mw:
        mw.set_polytopes(er.polytopes())
        mw.upload(bodies, sid, 0, len(bodies))
        for _ in range(frames):
            mw.step(dt, substeps)
        stats = mw.plan_stats()
        got = mw.download()
    assert stats["plans"] >= 2 and stats["migrated"] + stats["full_plans"] > 0, stats
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(er.polytopes())
        w.upload(bodies, sid)
        for _ in range(frames):
            w.step(dt, substeps)
        one = w.download()
        assert w.contact_stats()[0] == 0
    assert bits_equal(got, one)
    assert bits_equal(got, states[-1][sel])


@pytest.mark.parametrize("substeps", [1, 20])
def test_exact_heights_bit_for_bit(substeps):
    bodies, sid, verts, off, _ = er.exact_heights()
    want, want_masks = ob.step_bodies(bodies, sid, verts, off, 1.0 / 60.0, substeps, want_masks=True)
    nan = np.isnan(want)
    assert nan.any() and not nan.all()
    for mode in (capi.MODE_FUSED, capi.MODE_PER_SUBSTEP):
        with capi.World(mode=mode, trace_contacts=True) as w:
            w.set_shapes(verts, off)
            w.upload(bodies, sid)
            w.step(1.0 / 60.0, substeps)
            got, masks = w.download(), w.contact_masks(substeps)
        assert np.array_equal(masks, want_masks)
        assert np.array_equal(np.isnan(got), nan)
        assert bits_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want))
    one = np.array([capi.step_one(b, verts, 1.0 / 60.0, substeps) for b in bodies])
    assert np.array_equal(np.isnan(one), nan) and bits_equal(np.where(nan, 0.0, one), np.where(nan, 0.0, want))
