"""The f64 oracle of the body-body contact extension (oracle/xpbd_pairs_oracle.c, with materials tests/material_model.py)
against an independent extended-precision model (tests/xprec_pairs_model.py): manifolds (stage N), one contacts substep on
the oracle's manifolds (stage S) and on the model's own (stage S o N); physical checks on the model itself; and a mutation
check that the bound sees each class of misreading.  Scenes, bound, exclusions and measured constants: xprec_pairs_cases.py."""
import numpy as np
import pytest

import oracle_binding as ob
import xprec_cases as xc
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm

SCENE_NAMES = list(pc.SCENES)


def random_pairs(count, seed):
    polys, shapes, _ = pc.table()
    rng = np.random.default_rng(seed)
    kinds = (pc.CUBE, pc.TETRA, pc.ICOSA, pc.HULL16, pc.HULL18)
    for _ in range(count):
        ka, kb = (kinds[k] for k in rng.integers(0, len(kinds), 2))
        qa, qb = pc.random_rotation(rng), pc.random_rotation(rng)
        pa = rng.uniform(-1, 1, 3)
        pb = pa + rng.normal(size=3) * 0.45
        yield (pa, qa), (pb, qb), ka, kb


def test_stage_n_against_the_sat_on_random_pairs():
    """2 000 random pairs over the five shape classes: every decided query gives the oracle's verdict, feature, faces or
    supporting edges and point count, and its separation and points within K_MANIFOLD."""
    polys, shapes, _ = pc.table()
    worst, undecided, feats, touching = 0.0, 0, set(), 0
    for fa, fb, ka, kb in random_pairs(2000, 0):
        o = ob.sat(fa, fb, polys[ka], polys[kb])
        m = pm.manifold(fa, fb, shapes[ka], shapes[kb])
        if not pm.decided(m, pc.TAU):
            undecided += 1
            continue
        scale = max(np.linalg.norm(fa[0]), np.linalg.norm(fb[0])) + max(shapes[ka]["radius"], shapes[kb]["radius"])
        what, err = pc.compare_manifold(m, o, polys[ka], polys[kb], scale)
        assert what is None, (what, ka, kb, m["margins"])
        worst = max(worst, err)
        if m["p_ref"]:
            touching += 1
            feats.add(m["feature"])
    print("random pairs: touching %d, undecided %d, worst normalised error %.2f" % (touching, undecided, worst))
    assert worst <= pc.K_MANIFOLD
    assert feats == {pm.FACE_A, pm.FACE_B, pm.EDGES} and touching > 500 and undecided < 20


EPA_DEPTH_TOL, EPA_NORMAL_TOL, AXIS_UNIQUE = pc.EPA_DEPTH_TOL, pc.EPA_NORMAL_TOL, pc.AXIS_UNIQUE


def test_stage_n_against_gjk_epa_verdict_depth_and_normal():
    """EPA's depth is minus the largest query and its normal that query's axis, from A towards B: 600 random pairs.  The
    normal is compared where the best axis leads every other axis by more than AXIS_UNIQUE metres."""
    polys, shapes, _ = pc.table()
    checked = normals = 0
    for fa, fb, ka, kb in random_pairs(600, 1):
        r = ob.gjk_epa(fa, fb, polys[ka], polys[kb])
        m = pm.manifold(fa, fb, shapes[ka], shapes[kb])
        if m["margins"]["touch"] <= 1e-7 or r.status == ob.GJK_DEGENERATE:
            continue
        assert (r.status == ob.GJK_PENETRATING) == (not m["separated"]), (ka, kb, m["margins"])
        if m["separated"]:
            continue
        assert abs(r.depth - float(m["depth"])) <= EPA_DEPTH_TOL, (r.depth, float(m["depth"]))
        checked += 1
        if m["margins"]["axis"] > AXIS_UNIQUE:
            axis = xm.native().to_f64(m["axis"])
            assert np.abs(r.normal.np() - axis).max() <= EPA_NORMAL_TOL, (ka, kb, r.normal.np(), axis, m["margins"])
            normals += 1
    print("EPA: %d depths, %d normals compared" % (checked, normals))
    assert checked > 150 and normals > 120


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_oracle_against_the_model_substep_by_substep(name):
    """Every substep re-seeds the model from the oracle's f64 state: decided manifolds agree (discrete fields equal,
    separation and points within K_MANIFOLD), no pair the model finds touching is missing from the oracle's neighbour
    lists, and every checked body-substep is within K_PAIRS for stage S on the oracle's manifolds and for stage S o N.
    At most 10 % of the touching pair queries and of the body-substeps are excluded, and every feature stays checked."""
    t = pc.trajectory(name)
    polys, sid = pc.table()[0], t["sid"]
    wants = [fr[1] for fr in t["frames"]]
    errs_given, _ = pc.check_states(name, wants, "given")
    errs, excl = pc.check_states(name, wants, "res")
    touching = left_out = 0
    worst, feats = 0.0, {}
    for f, (start, want, frames, oman, res, given, _) in enumerate(t["frames"]):
        for key, m in res["manifolds"].items():
            i, j = key
            if m["p_ref"]:
                touching += 1
            if key in res["undecided"]:
                left_out += bool(m["p_ref"])
                continue
            if m["p_ref"] and m["margins"]["touch"] > pc.TAU:
                assert key in oman, "%s substep %d: the oracle never tested the touching pair %s" % (name, f, key)
            if key not in oman:
                continue
            scale = max(np.linalg.norm(frames[i][0]), np.linalg.norm(frames[j][0])) + max(t["ext"][i], t["ext"][j])
            what, err = pc.compare_manifold(m, oman[key], polys[int(sid[i])], polys[int(sid[j])], scale)
            assert what is None, "%s substep %d pair %s: %s (margins %s)" % (name, f, key, what, m["margins"])
            assert err <= pc.K_MANIFOLD, (name, f, key, err)
            worst = max(worst, err)
            if m["p_ref"]:
                feats[(t["labels"][i], m["feature"])] = feats.get((t["labels"][i], m["feature"]), 0) + 1
        for key, o in oman.items():
            if not o.separated and o.n_points and key not in res["undecided"]:
                assert key in res["manifolds"], "%s substep %d: pair %s touches in the oracle alone" % (name, f, key)
    print("%s: S o N %.1f, S %.1f, manifolds %.2f; excluded %d of %d body-substeps, %d of %d touching queries; %s" % (
        name, np.where(excl, 0, errs).max(), np.where(excl, 0, errs_given).max(), worst, excl.sum(), excl.size, left_out, touching,
        sorted(feats.items())))
    in_contact = np.zeros(excl.shape, dtype=bool)                        # the body-substeps that touch a pair: free flight
    for f, fr in enumerate(t["frames"]):                                 # must not dilute the cap
        for (i, j), m in fr[4]["manifolds"].items():
            if m["p_ref"]:
                in_contact[f, [i, j]] = True
    print("%s: %d of %d touching body-substeps excluded" % (name, (excl & in_contact).sum(), in_contact.sum()))
    assert touching >= 6
    assert left_out <= 0.10 * touching and excl.mean() <= 0.10 and (excl & in_contact).sum() <= 0.10 * in_contact.sum()
    kinds = {k for (_, k) in feats}
    if name.startswith(("general", "edge", "pile")):
        assert kinds == {pm.FACE_A, pm.FACE_B, pm.EDGES}
    elif name.startswith("crossed"):
        assert kinds == {pm.EDGES}
    else:
        assert kinds == {pm.FACE_A}                                       # exact ties: the reference face goes to A
    if name.startswith("edge"):
        for cat in pc.EDGE_CATEGORIES + ("slab",):
            assert any(label == cat for (label, _) in feats), cat         # every category keeps a checked touching pair


GJK_SCENES = [n for n in SCENE_NAMES if n.startswith(("general", "aligned", "pile")) and pc.SCENES[n][3] is None]


@pytest.mark.parametrize("name", GJK_SCENES)
def test_gjk_epa_oracle_against_the_model_substep_by_substep(name):
    """OP_NARROWPHASE_GJK_EPA on scenes (a), (b) and the friction-free pile of (e) (tests/material_model.py, the f64
    definition with friction, has the SAT only): every body-substep whose manifolds are face-aligned clips or EPA points
    that stage N reproduces by depth and normal is within K_PAIRS of stage S on them; at least half of the body-substeps
    that touch a pair are of that kind (measured: 95 %, 87 %, 100 %, 100 %, 70 %)."""
    checked, total = pc.check_gjk_states(name, [fr[1] for fr in pc.gjk_trajectory(name)])
    print("%s under GJK + EPA: %d of %d touching body-substeps checked" % (name, checked, total))
    assert total >= 50 and checked >= 0.5 * total


@pytest.mark.parametrize("name", ["aligned-h1200", "aligned-h240", "edge-h1200", "edge-h240"])
def test_longdouble_model_equals_mpmath_model(name):
    """Scenes (b) and (d), the substep that holds the scene's largest error of the oracle against the longdouble model, in
    longdouble and in 40-digit mpmath: the same manifolds, and states 2^11 times inside K_PAIRS, far below 10 % of that
    maximum: the longdouble model's own rounding does not set the measured maxima."""
    fast, ref = xm.native(), xm.mp(40)
    t = pc.trajectory(name)
    errs, excl = pc.check_states(name, [fr[1] for fr in t["frames"]])
    worst = int(np.where(excl, 0, errs).max(axis=1).argmax())
    bodies, sid, h, mu, ground_mu, speed = t["frames"][worst][0], t["sid"], t["h"], t["mu"], t["ground_mu"], t["speed"]
    shapes = pc.table()[1]
    a = pm.substep(bodies, shapes, sid, h, None, mu, ground_mu, speed, num=fast)
    b = pm.substep(bodies, shapes, sid, h, None, mu, ground_mu, speed, num=ref)
    assert sorted(a["manifolds"]) == sorted(b["manifolds"]) and a["manifolds"]
    for key, m in a["manifolds"].items():
        w = b["manifolds"][key]
        assert (m["feature"], m["index_a"], m["index_b"], len(m["p_ref"])) == (w["feature"], w["index_a"], w["index_b"], len(w["p_ref"]))
    hi = a["state"].astype(np.float64)                           # longdouble -> mpf exactly: two doubles
    lo = (a["state"] - hi.astype(a["state"].dtype)).astype(np.float64)
    d = np.abs(ref.to_f64(ref.conv(hi) + ref.conv(lo) - b["state"]))
    ext = pc.extents(sid, bodies)
    scale = pc.scales(bodies, hi, ext, list(a["manifolds"]))
    turn = scale / ext
    e = np.max(np.stack([d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * turn),
                         d[:, 22:25].max(axis=1) * h / (pc.EPS * scale), d[:, 25:28].max(axis=1) * h / (pc.EPS * turn)]), axis=0)
    print("%s substep %d: longdouble against mpmath %.4f, oracle against longdouble %.1f" % (name, worst, e.max(), errs[worst].max()))
    assert e.max() <= pc.K_PAIRS / 2 ** 11 and e.max() <= 0.1 * np.where(excl, 0, errs).max()


def isolated_pair(seed):
    rng = np.random.default_rng(seed)
    a = pc.new_body(pc.CUBE, (0.3, -0.2, 5.0), pc.random_rotation(rng), rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3), gravity=False)
    b = pc.new_body(pc.ICOSA, (0.0, 0.0, 0.0), pc.random_rotation(rng), rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3), gravity=False)
    pc.touch(a, pc.CUBE, b, pc.ICOSA, rng.normal(size=3), 0.01)
    return np.array([a, b]), np.array([pc.CUBE, pc.ICOSA], dtype=np.uint32)


def momenta(num, before, after, state0):
    """Sum of m dx and of m x cross dx + I dtheta over the bodies, from the pose change of the pair solve alone (the poses
    after integrate are `before`); dtheta is twice the vector part of dq q^-1."""
    lin, ang = 0, 0
    for k in range(len(state0)):
        m = 1.0 / state0[k, 0]
        inv = state0[k, 1:10].reshape(3, 3).T                               # [row, col]
        x0 = before[k, 31:34] + before[k, 28:31]
        dx = after[k, 31:34] - before[k, 31:34]
        dq = xm.qmul(after[k, 34:38][:, None], xm.conj(before[k, 34:38][:, None]))[:, 0]
        dtheta = dq[1:] * 2
        lin = lin + dx * m
        ang = ang + np.cross(x0, dx) * m + np.linalg.solve(inv, num.to_f64(dtheta))
    return num.to_f64(lin), num.to_f64(ang)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_conserves_momentum_on_an_isolated_pair(seed):
    """No gravity, no ground, bodies at rest (no tangential term: dir is along the correction): the corrections of a
    touching pair are +-lambda dir at two points of one line, so sum m dx vanishes to rounding, and the angular sum
    m x cross dx + I dtheta vanishes to first order.  What is left is second order in the turn: dtheta is read back from
    a normalised q + (0, theta / 2) q, and the Jacobi average adds the spins of points at different arms; with turns
    of 1e-3 rad that is 1e-6 of the linear momentum moved (measured: 9e-7 at most), and the test allows 1e-5.  A wrong arm
    (no centre of mass) gives 0.1.  Cube and icosahedron have isotropic inertia, and must: Rigid::apply_impulse turns by
    (M arm) x impulse (rigid.rs:118-122), which is M (arm x impulse), the conserved form, only for M = k 1; for any other
    inverse inertia the reference itself does not conserve angular momentum, so this check cannot be made there (the
    transposed-inertia mutation and scene (d) cover those bodies against the oracle instead)."""
    num = xm.native()
    bodies, sid = isolated_pair(seed)
    shapes = pc.table()[1]
    h = pc.HS[0]
    still = bodies.copy()
    still[:, 22:28] = 0.0
    res = pm.substep(still, shapes, sid, h)
    assert any(m["p_ref"] for m in res["manifolds"].values())
    before = num.conv(still)
    lin, ang = momenta(num, before, res["state"], still)
    moved = np.abs(num.to_f64(res["state"][:, 31:34] - before[:, 31:34])).max() / still[:, 0].min()
    assert moved > 1e-4
    assert np.abs(lin).max() <= 1e-15 * moved, (lin, moved)
    assert np.abs(ang).max() <= 1e-5 * moved, (ang, moved)


@pytest.mark.parametrize("seed", [1, 2])
def test_model_mirrors_when_a_and_b_are_swapped(seed):
    num = xm.native()
    bodies, sid = isolated_pair(seed)
    shapes = pc.table()[1]
    one = pm.substep(bodies, shapes, sid, pc.HS[1])
    two = pm.substep(bodies[::-1].copy(), shapes, sid[::-1].copy(), pc.HS[1])
    (m1,), (m2,) = one["manifolds"].values(), two["manifolds"].values()
    assert m1["p_ref"] and len(m1["p_ref"]) == len(m2["p_ref"])
    if m1["feature"] != pm.EDGES:
        assert m2["feature"] == 1 - m1["feature"] and (m2["index_a"], m2["index_b"]) == (m1["index_b"], m1["index_a"])
    d = np.abs(num.to_f64(one["state"] - two["state"][::-1]))
    assert d[:, 31:38].max() <= 1e-15 and d[:, 22:28].max() <= 1e-15 / pc.HS[1], d.max()


def test_model_moves_with_a_binary_exact_rigid_motion():
    """A quarter turn about z and a shift by (64, -32, 16) m: exact in f64, so the model's result (position, rotation
    qz * q, velocity and angular velocity R w) turns and shifts with it to its own rounding."""
    num = xm.native()
    bodies, sid = isolated_pair(4)
    shapes = pc.table()[1]
    moved = bodies.copy()
    r = np.sqrt(0.5)
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    shift = np.array([64.0, -32.0, 16.0])
    # the body keeps its shape frame: position' = R (position + com) - com + shift, rotation' = qz * rotation
    for k in range(2):
        moved[k, 31:34] = turn @ (bodies[k, 31:34] + bodies[k, 28:31]) - bodies[k, 28:31] + shift
        moved[k, 22:25], moved[k, 25:28] = turn @ bodies[k, 22:25], turn @ bodies[k, 25:28]
        moved[k, 34:38] = xm.qmul(np.array([r, 0.0, 0.0, r])[:, None], bodies[k, 34:38][:, None])[:, 0]
    one = num.to_f64(pm.substep(bodies, shapes, sid, pc.HS[0])["state"])
    two = num.to_f64(pm.substep(moved, shapes, sid, pc.HS[0])["state"])
    for k in range(2):
        want = turn @ (one[k, 31:34] + one[k, 28:31]) - one[k, 28:31] + shift
        assert np.abs(two[k, 31:34] - want).max() <= 1e-13                # sqrt(1/2) is rounded: eps |x| of the shifted pose
        assert np.abs(two[k, 22:25] - turn @ one[k, 22:25]).max() <= 1e-13 / pc.HS[0]
        want_q = xm.qmul(np.array([r, 0.0, 0.0, r])[:, None], one[k, 34:38][:, None])[:, 0]
        assert np.abs(two[k, 34:38] - want_q).max() <= 1e-13
        assert np.abs(two[k, 25:28] - turn @ one[k, 25:28]).max() <= 1e-13 / pc.HS[0]


# The first scene (in SCENES order) whose oracle trajectory leaves the bound of each deliberately wrong model.  general-h1200
# is the first scene of all; the scenes before edge-h1200 hold only bodies of symmetric inverse inertia, on which the
# transposed variant is the model itself, and pile-h240-mu is the first scene with finite friction.
CAUGHT_BY = {"reference_sign": "general-h1200", "arm_without_com": "general-h1200", "transposed_inertia": "edge-h1200",
             "average_by_pairs": "general-h1200", "friction_against_distance": "pile-h240-mu", "tangential_dropped": "general-h1200"}


@pytest.mark.parametrize("mutation", pm.MUTATIONS)
def test_the_bound_sees_each_misreading(mutation):
    """Each wrong variant of the MODEL pushes the oracle beyond K_PAIRS on the named scene, on a body-substep that the
    true model checks: the bound can see that class of mistake."""
    name = CAUGHT_BY[mutation]
    t = pc.trajectory(name)
    shapes = pc.table()[1]
    worst = 0.0
    for start, want, _, _, res, _, _ in t["frames"]:
        if not res["manifolds"]:
            continue
        wrong = pm.substep(start, shapes, t["sid"], t["h"], res["manifolds"], t["mu"], t["ground_mu"], t["speed"], mutation=mutation)
        e = pc.normalized_errors(want, wrong["state"], start, t["ext"], t["h"], list(res["manifolds"]))
        worst = max(worst, np.where(pc.excluded(res), 0.0, e).max())
    print("%s on %s: %.3g x the bound" % (mutation, name, worst / pc.K_PAIRS))
    assert worst > pc.K_PAIRS
