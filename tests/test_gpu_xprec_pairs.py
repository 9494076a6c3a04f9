"""The body-body contact scenes of tests/xprec_pairs_cases.py through the C ABI: the SAT narrowphase and the single-substep
contact trajectories, bit for bit against the oracle and, directly and not only by transitivity, within the
extended-precision model's bounds (K_MANIFOLD, K_PAIRS).  The edge categories of scene (d) (asymmetric inertia, offset
centre of mass, inverse mass 0 and 1e+-6, |x| = 1e4 m, fast spin) meet the pair solve here."""
import numpy as np
import pytest

import xprec_device as xd
import xprec_pairs_cases as pc
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(pc.SCENES)


def run(name, **kw):
    """Every single-substep frame of the scene on the device, each from the oracle's state at its start (for (b): from its
    fresh exact configuration)."""
    t = pc.trajectory(name)
    return t, xd.run_frames([(fr[0], t) for fr in t["frames"]], **kw)


def assert_oracle(t, got):
    for f, fr in enumerate(t["frames"]):
        assert bits_equal(got[f], fr[1]), "state differs from the oracle in substep %d" % f


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_narrowphase_on_the_scenes_frames(name):
    """World.narrowphase on the post-integrate frames of every substep, for the oracle's neighbour pairs: the oracle's bits,
    and within K_MANIFOLD of stage N where the model's decisions have a margin.  Once more with the pair list repeated
    beyond 32 768 + 3 000 entries (the eight-pairs-per-wave class for box-like shapes): the same records."""
    t = pc.trajectory(name)
    polys, sid = pc.table()[0], t["sid"]
    checked, tiled = 0, False
    with capi.World() as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        for f, (_, _, frames, oman, res, _, moved) in enumerate(t["frames"]):
            if not oman:
                continue
            pairs = np.array(sorted(oman), dtype=np.uint32)
            w.upload(moved, sid)
            got = w.narrowphase(pairs)
            if not tiled:
                tiled = True
                many = np.tile(pairs, (-(-(32768 + 3000) // len(pairs)), 1))
                again = w.narrowphase(many)
                assert again.tobytes() == np.tile(got, len(many) // len(pairs)).tobytes()
            for g, key in zip(got, map(tuple, pairs)):
                o = oman[key]
                i, j = key
                if o.separated or o.n_points == 0:
                    assert g["n_points"] == 0
                else:
                    assert (g["n_points"], g["feature"], g["index_a"], g["index_b"]) == (o.n_points, o.feature, o.index_a, o.index_b)
                    ref, inc = o.points()
                    assert bits_equal(np.array([g["separation"]]), np.array([o.separation]))
                    assert bits_equal(g["p_ref"][:o.n_points], ref) and bits_equal(g["p_inc"][:o.n_points], inc)
                m = res["manifolds"].get(key)
                if m is None or key in res["undecided"]:
                    continue
                scale = max(np.linalg.norm(frames[i][0]), np.linalg.norm(frames[j][0])) + max(t["ext"][i], t["ext"][j])
                what, err = pc.compare_manifold(m, g, polys[int(sid[i])], polys[int(sid[j])], scale)
                assert what is None and err <= pc.K_MANIFOLD, (name, f, key, what, err)
                checked += bool(m["p_ref"])
    assert checked >= 6 and tiled


@pytest.mark.parametrize("schedule", xd.SAT_SCHEDULES, ids=xd.SCHEDULE_IDS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sat_trajectories(name, schedule):
    """MODE_CONTACTS, SAT, every schedule; the pile scenes with set_materials and set_max_depenetration_speed."""
    t, got = run(name, schedule=schedule)
    assert_oracle(t, got)
    pc.check_states(name, got)


@pytest.mark.parametrize("name", [s for s in SCENE_NAMES if s.startswith(("general", "aligned", "pile")) and pc.SCENES[s][3] is None])
def test_gjk_epa_trajectories(name):
    """GJK + EPA on scenes (a), (b) and the friction-free pile (the f64 definition with friction, tests/material_model.py,
    has the SAT only): the oracle's bits, and within K_PAIRS of stage S on the manifolds the model can reproduce (a
    face-aligned clip, or an EPA point whose depth and normal are stage N's) on at least half of the touching body-substeps."""
    t = pc.trajectory(name)
    got = []
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        w.set_narrowphase(capi.NARROWPHASE_GJK_EPA)
        for f, (start, want, *_) in enumerate(pc.gjk_trajectory(name)):
            w.upload(start, t["sid"])
            if t["speed"]:
                w.set_max_depenetration_speed(t["speed"])
            w.step(t["h"], 1)
            got.append(w.download())
            assert bits_equal(got[-1], want), f
    checked, total = pc.check_gjk_states(name, got)
    assert total >= 50 and checked >= 0.5 * total


@pytest.mark.parametrize("name", [s for s in SCENE_NAMES if s.startswith("pile")])
def test_pile_behind_a_far_field_uses_one_lane_per_body(name):
    t, got = run(name, far=xd.SMALL_WORLD + 16)
    assert_oracle(t, got)
    pc.check_states(name, got)


@pytest.mark.parametrize("name", [s for s in SCENE_NAMES if s.startswith("edge")])
def test_edge_categories_meet_the_pair_solve(name):
    """The device equals the oracle on scene (d), and every category has touching pairs by the device's own narrowphase
    at the post-integrate frames."""
    t, got = run(name)
    assert_oracle(t, got)
    touched = set()
    with capi.World() as w:
        w.set_polytopes(pc.capi_polytopes(capi))
        for _, _, _, oman, _, _, integrated in t["frames"]:
            pairs = np.array(sorted(oman), dtype=np.uint32).reshape(-1, 2)
            if len(pairs):
                w.upload(integrated, t["sid"])
                touched |= {t["labels"][i] for (i, _), g in zip(pairs, w.narrowphase(pairs)) if g["n_points"]}
    assert touched == set(pc.EDGE_CATEGORIES) | {"slab"}
