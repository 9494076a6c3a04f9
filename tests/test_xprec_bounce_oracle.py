"""Restitution (stage 6) and the terrain as ground: the f64 evaluation of the model against the extended-precision model
(xprec_pairs_model.substep with restitution=, ground_restitution=, bounce_threshold= and terrain=), frame by frame; the
existing f64 models (tests/restitution_model.py, tests/terrain_model.py) on their own joint-free scenes within the same bound;
the 40-digit model on the frames that hold the maxima; a mutation table; the caps and "seen both ways" conditions of the scene
set; and mechanics of the model itself.  Scenes, bound, exclusions and the measured figures: xprec_bounce_cases.py."""
import numpy as np
import pytest

import oracle_binding as ob
import restitution_model as rm
import terrain_model as tm
import xprec_bounce_cases as bc
import xprec_check as xk
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, pile

SCENE_NAMES = list(bc.SCENES)


def f64_states(name):
    return [fr[1] for fr in bc.trajectory(name)["frames"]]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_f64_reading_against_the_model_frame_by_frame(name):
    """Every checked body-substep of the f64 evaluation of the model is within K_BOUNCE of the longdouble model; the exclusion
    caps hold over all body-substeps and over those that carry a stage-6 entry (scene (g): a terrain contact).  The exact
    scenes add no entry where the header says none."""
    t = bc.trajectory(name)
    errs, excl, entry = bc.check_states(name, f64_states(name))
    x, c = np.concatenate(excl), np.concatenate(entry)
    print("%s: f64 evaluation %.1f; excluded %d of %d body-substeps, %d of %d with a stage-6 entry%s" % (
        name, xk.worst(errs, excl), x.sum(), x.size, (x & c).sum(), c.sum(), " (terrain contact)" if name.startswith("terrain") else ""))
    xk.assert_caps(name, excl, entry)
    for f, (start, want, res, s) in enumerate(t["frames"]):
        assert len(start) <= bc.MAX_BODIES and not np.isnan(want).any()
        if name.startswith("exact"):
            assert res["bounce_pair_entries"].tolist() == bc.EXACT_PAIR_ENTRIES, f
            assert (res["bounce_ground_entries"] > 0).tolist() == bc.EXACT_GROUND, f
            assert res["mask"][[5, 6, 7]].all() and res["n_points"][[0, 1, 3, 4, 10, 11]].all()      # the contacts are there
            assert res["threshold_margin"][[3, 4, 5]].tolist() == [0.0, 0.0, 0.0]                    # vn0 == -threshold exactly
            assert bits_equal(want[[8, 10]], start[[8, 10]])                                         # immovable, and no NaN
        if name.startswith("grid"):
            assert res["mask"][0] == 0 and res["margin"][0] == 0.0                                   # s == 0 exactly: no contact
            assert bin(int(res["mask"][1])).count("1") == 1 and res["n_outside"][:2].tolist() == [0, 6]
            assert res["mask"][3] != 0 and res["bounce_ground_entries"][3] == 0                     # `edge`: pushed out of the field
            assert res["cell_margin"][1] == 0.0 and res["diagonal_margin"][1] == 0.0 and res["border_margin"][0] == 0.0
            assert bits_equal(want[0], start[0])
        if name.startswith("cell"):
            assert bin(int(res["mask"][0])).count("1") >= 1 and res["diagonal_margin"][0] == 0.0 and res["n_outside"][0] == 0
        if name.startswith("zero"):
            assert not res["n_outside"].any()
    if name.startswith("terrain"):
        over = sum((fr[2]["mask"] != 0) for fr in t["frames"])
        outside = sum(fr[2]["n_outside"] for fr in t["frames"])
        counts = np.array([len(pc.table()[1][int(k)]["verts"]) for k in t["frames"][0][3]["sid"]]) * len(t["frames"])
        # some bodies over the field, some straddling its border, some beyond it
        assert (outside == 0).sum() >= 5 and ((outside > 0) & (outside < counts)).sum() >= 3 and (outside == counts).sum() >= 5
        assert (over > 0).sum() >= 4
    if name.startswith("ends"):
        labels = t["frames"][0][3]["labels"]
        carried = np.zeros(len(labels), dtype=bool)
        for f in range(len(t["frames"])):
            carried |= entry[f] & ~excl[f]
        for cat in pc.EDGE_CATEGORIES + ("slab",):
            assert carried[labels == cat].any(), cat                     # every category is checked with a stage-6 entry
        assert {1e-6, 1e6} <= set(t["frames"][0][0][labels == "mass_extreme"][:, 0].tolist())
    if name.startswith(("chain", "limits", "lifts", "wheels")):
        jointed = sum((fr[2]["n_joint"] > 0) & bc.carries(name, fr[2]) & (fr[0][:, 0] > 0) for fr in t["frames"])
        assert (jointed > 0).sum() >= (8 if name.startswith("chain") else 4), jointed       # jointed bodies bounce
    if name.startswith("jointed"):
        jointed = sum((fr[2]["n_joint"] > 0) & bc.carries(name, fr[2]) for fr in t["frames"])
        driven = sum((fr[2]["n_extra"] > 0) & bc.carries(name, fr[2]) for fr in t["frames"])
        assert jointed.sum() >= 100 and driven.sum() >= 20               # jointed and driven bodies bounce
    if name.startswith("faces"):
        sizes, idle_frames = set(), 0
        for fr in t["frames"]:
            sizes |= {len(m["p_ref"]) for m in fr[2]["manifolds"].values()}
            stack = np.nonzero(fr[3]["labels"] == "stack")[0]
            assert fr[2]["bounce_pair_entries"][stack].max() == 2        # the middle box averages two manifolds
            idle = np.nonzero(fr[3]["labels"] == "idle")[0]
            assert (fr[2]["n_points"][idle] > 0).all()
            idle_frames += fr[2]["bounce_pair_entries"][idle].tolist() == [0, 1, 1]    # an idle manifold beside an active one
        assert {1, 2, 4} <= sizes and idle_frames >= len(t["frames"]) // 2


def test_the_bounds_are_eight_times_the_measured_maxima():
    """8x the largest measured error of the f64 evaluation does not fit under K_PAIRS (xprec_bounce_cases.py says which bodies
    and why).  K_BOUNCE is 8x the maximum over the bodies with a stage-6 entry from a one-point manifold, K_PLAIN 8x the
    maximum over all others; each holds its maximum and is no wider, and outside scene (d) the others stay under K_PAIRS / 8."""
    with_one, others, elsewhere = 0.0, 0.0, 0.0
    for name in SCENE_NAMES:
        a = b = 0.0
        for f, (start, want, res, s) in enumerate(bc.trajectory(name)["frames"]):
            e = np.where(bc.excluded(res, s["exact"]), 0, bc.errors(name, f, want, res))
            a, b = max(a, e[bc.one_point(res)].max(initial=0.0)), max(b, e[~bc.one_point(res)].max(initial=0.0))
        print("%s: %.1f with a one-point entry, %.1f without" % (name, a, b))
        with_one, others = max(with_one, a), max(others, b)
        elsewhere = max(elsewhere, 0.0 if name.startswith("ends") else b)
    print("largest normalised errors: %.1f (8x = %.0f, K_BOUNCE = %g), %.1f without a one-point entry (8x = %.0f, K_PLAIN = %g), "
          "%.1f of that outside scene (d)" % (with_one, 8 * with_one, bc.K_BOUNCE, others, 8 * others, bc.K_PLAIN, elsewhere))
    assert 8 * with_one <= bc.K_BOUNCE <= 8.01 * with_one
    assert 8 * others <= bc.K_PLAIN <= 8.01 * others
    assert 8 * elsewhere <= pc.K_PAIRS


def test_every_joint_limit_and_drive_kind_meets_stage_6():
    """On a checked body, in the very substep in which it has a stage-6 entry: every joint kind, the perpendicular term, a
    binding HINGE, SWING, TWIST and SLIDE limit, and an acting drive of each of the four kinds."""
    kinds = bc.kinds_with_entry([n for n in SCENE_NAMES if n.startswith(("jointed", "chain", "limits", "lifts", "wheels"))])
    print(sorted(kinds))
    want = {("joint", k) for k in (pm.JOINT_DISTANCE, pm.JOINT_HINGE, pm.JOINT_SLIDER)}
    want |= {("limit", k) for k in (pm.LIMIT_HINGE, pm.LIMIT_SWING, pm.LIMIT_TWIST)} | {("slide limit",), ("perpendicular",)}
    want |= {("drive", k) for k in (pm.DRIVE_ANGLE, pm.DRIVE_ANGULAR_VELOCITY, pm.DRIVE_POSITION, pm.DRIVE_VELOCITY)}
    assert want <= kinds, want - kinds


def test_the_scene_set_sees_everything_both_ways():
    tags = bc.seen(SCENE_NAMES)
    want = bc.SEEN_BOTH_WAYS | {"a terrain contact in a lower triangle", "a terrain contact in an upper triangle",
                                "a vertex outside the field"}
    assert want <= tags, want - tags


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_longdouble_model_equals_mpmath_model(name):
    """The frame that holds the scene's largest error, stage S and stage 6 on the longdouble model's manifolds, in longdouble
    and in 40-digit mpmath: the states agree 2^11 times inside K_BOUNCE and within a tenth of that maximum, and stage 6 makes
    the same entries: longdouble's rounding does not set the bound."""
    fast, ref = xm.native(), xm.mp(40)
    t = bc.trajectory(name)
    errs, excl, _ = bc.check_states(name, f64_states(name))
    per_frame = [float(np.where(x, 0, e).max()) for e, x in zip(errs, excl)]
    f = int(np.argmax(per_frame))
    start, _, res, s = t["frames"][f]
    given = {key: m for key, m in res["manifolds"].items() if m["p_ref"]}
    exact = {key: {"separated": False, "feature": m["feature"], "p_ref": [xm.lifted(ref, p) for p in m["p_ref"]],
                   "p_inc": [xm.lifted(ref, p) for p in m["p_inc"]], **({"normal": xm.lifted(ref, m["normal"])} if "normal" in m else {})}
             for key, m in given.items()}
    a = bc.model(name, f, num=fast, manifolds=given)
    b = bc.model(name, f, num=ref, manifolds=exact)
    for key in ("mask", "bounce_pair_entries", "bounce_ground_entries"):      # (a converged point's later visits are +-rounding)
        if key in a:
            assert np.array_equal(a[key], b[key]), key
    d = np.abs(ref.to_f64(xm.lifted(ref, a["state"]) - b["state"]))
    scale = pc.scales(start, fast.to_f64(a["state"]), s["ext"], xk.joint_links(s, res))
    turn = scale / s["ext"]
    h = s["h"]
    e = np.max(np.stack([d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * turn),
                         d[:, 22:25].max(axis=1) * h / (pc.EPS * scale), d[:, 25:28].max(axis=1) * h / (pc.EPS * turn)]), axis=0)
    print("%s frame %d: longdouble against mpmath %.4f = %.2g of the bound; the scene's maximum %.1f" % (
        name, f, e.max(), e.max() / bc.K_BOUNCE, per_frame[f]))
    assert e.max() <= bc.K_BOUNCE / 2 ** 11 and e.max() <= 0.1 * per_frame[f]


# The scene on which each wrong reading of the MODEL leaves the bound, and the measured factor (worst error / K_BOUNCE).
CAUGHT_BY = {"e_smaller_side": ("bounce-h240", 1.8e10), "vn0_post_derive": ("bounce-h240", 1.5e10),
             "threshold_on_vn": ("bounce-h240", 3.2e9), "arms_at_integrated": ("bounce-h240", 1.2e9),
             "points_averaged": ("faces-h240", 4.8e8), "one_sweep": ("faces-h240", 6.1e8), "no_give_back": ("faces-h240", 6.1e8),
             "entries_summed": ("faces-h240", 7.0e8), "idle_counted": ("faces-h240", 1.5e8),
             "reference_pushed_same_way": ("faces-h240", 2.8e10), "compliance_in_wsum": ("bounce-h1200", 1.4e9),
             "ground_before_pairs": ("bounce-h240", 2.5e10), "ground_reads_pre_ground": ("bounce-h240", 3.0e9),
             "impulse_arm_in_rest_space": ("bounce-h240", 3.7e11), "triangles_swapped": ("terrain-h240-off", 1.7e10),
             "target_vertical": ("terrain-h240-off", 1.1e10), "d_unnormalised": ("terrain-h240-off", 1.8e10),
             "plane_beyond_field": ("terrain-h240-off", 9.2e9), "bounce_normal_vertical": ("terrain-h240-on", 2.3e10),
             "bounce_lookup_at_integrated": ("grid-h240", 5.4e8)}
# Invisible where they cannot act: ground_reads_pre_ground on the terrain and the exact terrain scenes (1e-3 of the bound: a body's
# first bouncing vertex leaves the others with vn >= (-e) vn0, one entry per body and nothing to re-read), idle_counted on
# terrain-h1200-on (no body there has an idle manifold beside an active one; scene (b) has one by construction), and
# bounce_lookup_at_integrated on scene (g) and on `cell` (the position pass moves a vertex by millimetres: it stays in its
# triangle); on `grid` the contact vertex starts exactly on a grid corner and the solve moves it into the next cell.


@pytest.mark.parametrize("mutation", pm.BOUNCE_MUTATIONS)
def test_the_bound_sees_each_misreading(mutation):
    """Each wrong variant of the model pushes the f64 evaluation beyond K_BOUNCE on the named scene, on a body-substep that the
    true model checks."""
    name, factor = CAUGHT_BY[mutation]
    t = bc.trajectory(name)
    worst = 0.0
    for f, (start, want, res, s) in enumerate(t["frames"]):
        wrong = bc.model(name, f, mutation=mutation, manifolds=res["manifolds"])
        worst = max(worst, np.where(bc.excluded(res, s["exact"]), 0.0, bc.errors(name, f, want, wrong)).max())
    print("%s on %s: %.3g x the bound (recorded: %.2g)" % (mutation, name, worst / bc.K_BOUNCE, factor))
    assert worst > bc.K_BOUNCE


@pytest.mark.parametrize("name,without", [("bounce-h1200", "restitution"), ("faces-h1200", "restitution"),
                                          ("terrain-h1200-on", "terrain"), ("terrain-h1200-off", "terrain"),
                                          ("terrain-h1200-on", "flat")])
def test_the_bound_sees_restitution_and_the_terrain(name, without):
    """The model without restitution leaves the bound of the full model on scenes (a) and (b), the model without the terrain
    (and on a flattened field) on scene (g): the device controls of test_gpu_xprec_bounce.py, on the CPU reading."""
    t = bc.trajectory(name)
    worst = 0.0
    for f in range(2):
        _, _, res, s = t["frames"][f]
        less = bc.model(name, f, num=xm.f64(), without=(without,))
        worst = max(worst, np.where(bc.excluded(res, s["exact"]), 0, bc.errors(name, f, xm.f64().to_f64(less["state"]), res)).max())
    print("%s without %s: %.3g x the bound" % (name, without, worst / bc.K_BOUNCE))
    assert worst > bc.K_BOUNCE


# ---- mechanics of the model itself ----------------------------------------------------------------------------------------
def head_on(e, h=pc.HS[0]):
    """Two free cubes far from the ground, no forces, face to face along x, 0.1 mm apart, closing at 2 m/s in all."""
    a = pc.new_body(pc.CUBE, (0.0, 0.0, 8.0), velocity=(1.0, 0.0, 0.0), gravity=False)
    b = pc.new_body(pc.CUBE, (1.0 + 1e-4, 0.03, 8.02), velocity=(-1.0, 0.0, 0.0), gravity=False)
    return np.array([a, b]), np.array([e, e])


@pytest.mark.parametrize("e", [1.0, 0.3])
def test_free_head_on_pair_keeps_its_momentum_and_leaves_at_e_times_the_closing_speed(e):
    """Stage 6 applies +lambda n and -lambda n: the linear momentum is conserved to rounding.  The four pushing points leave at
    e times their closing speed to the convergence of four sweeps over a four-point face contact (measured 2e-4 of the closing
    speed; 0.05 allowed); without stage 6 the pair leaves at what the position pass left, far from it."""
    num = xm.native()
    bodies, es = head_on(e)
    sid = np.zeros(2, dtype=np.uint32)
    res = pm.substep(bodies, pc.table()[1], sid, pc.HS[0], None, restitution=es)
    assert res["bounce_pair_entries"].tolist() == [1, 1] and res["bounce_push"][0] >= 4 and len(res["manifolds"][(0, 1)]["p_ref"]) == 4
    v = num.to_f64(res["state"][:, 22:25])
    m = 1.0 / bodies[:, 0]
    assert np.abs((v * m[:, None]).sum(axis=0)).max() <= 1e-15                                    # it was 0 before
    w = num.to_f64(res["state"][:, 25:28])
    leaving = []
    for p_ref, p_inc in zip(res["manifolds"][(0, 1)]["p_ref"], res["manifolds"][(0, 1)]["p_inc"]):
        c = num.to_f64(res["state"][:, 31:34] + res["state"][:, 28:31])
        ref, inc = (1, 0) if res["manifolds"][(0, 1)]["feature"] == pm.FACE_B else (0, 1)
        n = num.to_f64(res["manifolds"][(0, 1)]["normal"])
        u = (v[inc] + np.cross(w[inc], num.to_f64(p_inc) - c[inc])) - (v[ref] + np.cross(w[ref], num.to_f64(p_ref) - c[ref]))
        leaving.append(float(n @ u))
    print("e = %g: the points leave at %s of a closing speed of 2 m/s" % (e, np.round(np.array(leaving) / 2.0, 4)))
    assert np.abs(np.array(leaving) - e * 2.0).max() <= 0.05 * 2.0
    plain = pm.substep(bodies, pc.table()[1], sid, pc.HS[0], None)
    assert abs(float(num.to_f64(plain["state"][1, 22] - plain["state"][0, 22])) - e * 2.0) > 0.2


def test_the_model_never_applies_an_attractive_impulse():
    """Every point's total impulse after the last pass and every ground entry's lambda is >= 0, on every frame of every scene;
    the no_give_back and reference_pushed_same_way readings are not asked: the true model is."""
    smallest, count = np.inf, 0
    for name in SCENE_NAMES:
        for _, _, res, _ in bc.trajectory(name)["frames"]:
            if "bounce_impulses" in res and len(res["bounce_impulses"]):
                smallest, count = min(smallest, res["bounce_impulses"].min()), count + len(res["bounce_impulses"])
    print("%d impulses, the smallest %g" % (count, smallest))
    assert count > 3000 and smallest >= 0.0


@pytest.mark.parametrize("name", ["zero-h1200", "zero-h240"])
def test_a_zero_field_equals_the_plane(name):
    """The f64 evaluation over the all-zero field (odd spacing) equals the f64 evaluation on the plane bit for bit; the longdouble
    model's two results are equal too."""
    for f in range(bc.SUBSTEPS):
        on_field = bc.model(name, f, num=xm.f64())
        on_plane = bc.model(name, f, num=xm.f64(), without=("terrain",))
        assert not on_field["n_outside"].any() and on_field["mask"].any()
        assert bits_equal(xm.f64().to_f64(on_field["state"]), xm.f64().to_f64(on_plane["state"])), f
        assert np.array_equal(bc.trajectory(name)["frames"][f][2]["state"], bc.model(name, f, without=("terrain",))["state"])


# ---- the existing f64 models, held to this one ----------------------------------------------------------------------------
def against(model, polys, sid, h, substeps, **settings):
    """`model` (restitution_model.Model or terrain_model.Model) stepped `substeps` single substeps, each against this model
    from the same state.  Returns (largest normalised error of a checked body-substep, stage-6 entries, terrain or ground
    contacts, excluded, total)."""
    shapes = [pm.shape(p) for p in polys]
    r = np.array([np.linalg.norm(shapes[int(k)]["verts"], axis=1).max() for k in sid])
    ext = r + 2 * np.linalg.norm(model.bodies[:, 28:31], axis=1)
    worst, entries, contacts, left_out, total = 0.0, 0, 0, 0, 0
    for _ in range(substeps):
        start = model.bodies.copy()
        got = model.step(h, 1).copy()
        res = pm.substep(start, shapes, sid, h, None, tau=pc.TAU, **settings)
        e = pc.normalized_errors(got, res["state"], start, ext, h, list(res["manifolds"]))
        x = bc.excluded(res)
        worst = max(worst, float(np.where(x, 0, e).max()))
        if "bounce_pair_entries" in res:
            entries += int((res["bounce_pair_entries"] + res["bounce_ground_entries"]).sum())
        contacts += int((res["mask"] != 0).sum())
        left_out, total = left_out + int(x.sum()), total + x.size
    return worst, entries, contacts, left_out, total


@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 96, 3), (capi.SCENE_MIXED_DROP, 120, 5)])
def test_the_restitution_model_lies_within_the_bound(kind, n, seed):
    """tests/restitution_model.py on the 96-box and 120-mixed-body piles that the device is held to it on bit for bit
    (test_gpu_restitution.py), coefficients from {0, 0.3, 0.8, 1}, ground 0.5: after 12 substeps of its own, three substeps
    each against this model from the same state."""
    rng = np.random.default_rng(seed)
    bodies, sid = pile(capi, kind, n, seed, 4.0, 3.0)
    e = bc.ES[rng.integers(0, len(bc.ES), n)]
    polys = ob.polytopes_array(POLY_NAMES[kind])
    model = rm.Model(bodies, sid, polys, e, 0.5, 0.0, pad=0.02)
    model.step(1.0 / 60.0, 6)
    model.step(1.0 / 60.0, 6)
    worst, entries, _, left_out, total = against(model, polys, sid, 1.0 / 360.0, 3, restitution=e, ground_restitution=0.5)
    print("restitution_model against the model: %.1f, %d stage-6 entries, %d of %d body-substeps excluded" % (worst, entries, left_out, total))
    assert worst <= bc.K_BOUNCE and entries >= 40 and left_out <= 0.10 * total


def test_the_terrain_model_lies_within_the_bound():
    """tests/terrain_model.py on the bumpy-field scene the device is held to it on bit for bit (test_gpu_terrain.py: the 96-box
    pile, mixed friction, ground friction 0.4, the field under part of it), with restitution on as well."""
    kind, n, seed = capi.SCENE_BOXES_DROP, 96, 3
    rng = np.random.default_rng(seed)
    bodies, sid = pile(capi, kind, n, seed, 4.0, 3.0)
    bodies[:, 33] -= 0.4
    mu = pc.MUS[rng.integers(0, len(pc.MUS), n)]
    e = bc.ES[rng.integers(0, len(bc.ES), n)]
    heights, origin, cell = tm.bumpy_field(9, 7, 11), (-8.0, -1.5), (1.3, 1.1)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    model = tm.Model(bodies, sid, polys, tm.Terrain(heights, origin, cell), mu=mu, ground_mu=0.4, pad=0.02, e=e, ground_e=0.5)
    model.step(1.0 / 60.0, 6)
    model.step(1.0 / 60.0, 6)
    worst, entries, contacts, left_out, total = against(model, polys, sid, 1.0 / 360.0, 3, mu=mu, ground_mu=0.4, restitution=e,
                                                        ground_restitution=0.5, terrain=xm.heightfield(heights, origin, cell))
    print("terrain_model against the model: %.1f, %d terrain contacts, %d stage-6 entries, %d of %d body-substeps excluded" % (
        worst, contacts, entries, left_out, total))
    assert worst <= bc.K_BOUNCE and contacts >= 10 and entries >= 40 and left_out <= 0.10 * total
