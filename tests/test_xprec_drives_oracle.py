"""Sliders, SLIDE limits and joint drives in contact: the f64 evaluation of the model against the extended-precision model
(xprec_pairs_model.substep with joints=, limits= and drives=), substep by substep; tests/joint_drive_model.py's contact-free
scenes within the same bound; the 40-digit model on the substeps that hold the maxima; a mutation table; the caps and
"seen both ways" conditions of the scene set; and invariants of the model itself.  Scenes, bound, exclusions and the measured
figures: xprec_drives_cases.py."""
import numpy as np
import pytest

import joint_drive_model as jd
import xprec_check as xk
import xprec_drives_cases as dc
import xprec_joints_cases as jc
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from constraint_solver_amd import capi

SCENE_NAMES = list(dc.SCENES)
INF = float("inf")


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_f64_reading_against_the_model_substep_by_substep(name):
    """Every checked body-substep of the f64 evaluation of the model is within K_DRIVES of the longdouble model; the
    exclusion caps hold over all body-substeps and over those that carry both an extra entry and a pair or ground point."""
    t = dc.trajectory(name)
    errs, excl, mixed = dc.check_states(name, [fr[1] for fr in t["frames"]])
    x, c = np.concatenate(excl), np.concatenate(mixed)
    print("%s: f64 evaluation %.1f; excluded %d of %d body-substeps, %d of %d with extra entry and contact point" % (
        name, xk.worst(errs, excl), x.sum(), x.size, (x & c).sum(), c.sum()))
    xk.assert_caps(name, excl, mixed)
    assert len(t["sid"]) <= dc.MAX_BODIES
    dynamic = t["bodies"][:, 0] > 0
    driven = np.zeros(len(t["sid"]), dtype=bool)
    for fr in t["frames"]:
        driven |= fr[2]["n_extra"] > 0
    resting = sum(((fr[2]["n_points"] > 0) | (fr[2]["mask"] != 0))[driven & dynamic] for fr in t["frames"])
    # every driven or sliding body touches something in most frames (the box of scene (d)'s pair at |x| = 1e4 m in half of
    # them at h = 1/240: the pair is thrown off the ground together and drifts apart)
    assert (resting > len(t["frames"]) / 2).all() or (name == "ends-h240" and (resting >= len(t["frames"]) / 2).all()), resting
    if name.startswith("exact"):
        for _, _, res, _ in t["frames"]:                                 # the skips are taken, on bodies that carry pair points
            assert res["n_extra"].tolist() == [1, 1, 0, 1, 1, 0, 0] and (res["n_points"] > 0).all()
            assert res["n_joint"].tolist() == [1, 2, 1, 1, 1, 0, 0]      # unit 1's hinge: its positional entry alone
            assert [(k, length != 0) for k, length in res["perps"]] == [(0, False), (2, True), (3, False)]
            assert [(k, s, e) for k, s, e in res["slides"]] == [(0, 0.25, 0.0), (3, 0.0, 0.0)]
            assert {(i, e != 0) for i, _, e, _, _ in res["drives"]} == {(0, True), (1, False), (2, False), (3, False), (4, False)}
    if name.startswith("ends"):
        both = np.zeros(len(t["sid"]), dtype=bool)
        for fr in t["frames"]:
            both |= dc.both(fr[2]) & ~dc.excluded(fr[2])
        for cat in pc.EDGE_CATEGORIES + ("slab",):
            assert both[t["labels"] == cat].any(), cat                   # every category is checked with extra entry and contact
        extremes = t["bodies"][t["labels"] == "mass_extreme"][:, 0]
        assert {1e-6, 1e6} <= set(extremes.tolist())
    if name.startswith("lifts") or name.startswith("mixed"):
        index = {label: int(np.nonzero(t["labels"] == label)[0][0]) for label in ("stall", "lift", "ramp", "drag", "floor")}
        joint = {label: [k for k, j in enumerate(t["joints"]) if b in (j["body_a"], j["body_b"])][0] for label, b in index.items()}
        binds = {label: [e != 0 for fr in t["frames"] for (k, _, e) in fr[2]["slides"] if k == joint[label]] for label in joint}
        assert all(binds["ramp"]) and not any(binds["floor"])            # from the first frame; never
        assert not binds["drag"][0] and binds["drag"][-1]                # starts to bind within the frames
        on_ground = sum(fr[2]["mask"][index["floor"]] != 0 for fr in t["frames"])
        assert on_ground > len(t["frames"]) / 2                          # ground points: `past` lies a ground solve behind


def test_the_bound_is_eight_times_the_measured_maximum():
    """K_DRIVES is K_PAIRS: 8x the largest measured error of the f64 evaluation over all scenes fits under it."""
    worst = 0.0
    for name in SCENE_NAMES:
        t = dc.trajectory(name)
        for start, want, res, _ in t["frames"]:
            worst = max(worst, np.where(dc.excluded(res), 0, dc.errors(name, want, res, start)).max())
    print("largest normalised error of all scenes: %.1f; 8x = %.0f; K_DRIVES = %g" % (worst, 8 * worst, dc.K_DRIVES))
    assert 8 * worst <= dc.K_DRIVES and dc.K_DRIVES == pc.K_PAIRS


def test_the_scene_set_sees_every_extra_both_ways():
    """Over the scene set the perpendicular term, the SLIDE limit and each drive kind are seen binding and not binding, a
    drive entry clamped and unclamped; the wheel of (b) passes pi between two consecutive checked frames."""
    kinds, clamps = dc.seen(SCENE_NAMES)
    assert kinds == {(k, b) for k in ("perp", "slide", pm.DRIVE_ANGLE, pm.DRIVE_ANGULAR_VELOCITY, pm.DRIVE_POSITION,
                                      pm.DRIVE_VELOCITY) for b in (False, True)}
    assert clamps == {False, True}
    for name in SCENE_NAMES:
        if name.startswith("wheels"):
            frames = dc.crossing(name)
            print("%s: the wheel passes pi between frames %s and the next" % (name, frames))
            assert len(frames) == 1


def contact_free_scene(seed, n_bodies=6):
    """The recipe of test_gpu_joint_drives.random_driven_scene on this file's bodies: free cubes in a row 2 m apart 3 m up
    (nothing touches), tilted and spinning, no gravity; hinges and sliders with HINGE and SLIDE limits and drives of all four
    kinds, some soft, some force-limited, in a shuffled order."""
    rng = np.random.default_rng(2000 + seed)
    bodies, rows, lims, drvs = [], [], [], []
    for i in range(n_bodies):
        bodies.append(pc.new_body(pc.CUBE, (2.0 * i, 0.0, 3.0), jc.tilt(rng, 0.3), velocity=rng.normal(scale=0.3, size=3),
                                  spin=rng.normal(scale=4.0, size=3), gravity=False, static=seed % 2 == 1 and i == 0))
    for k in range(n_bodies - 1):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ref = np.cross(axis, rng.normal(size=3))
        ref /= np.linalg.norm(ref)
        is_slider = rng.uniform() < 0.5
        rows.append(dict(body_a=k, body_b=k + 1, anchor_a=(1.5, 0.5, 0.5), anchor_b=(-0.5, 0.5, 0.5), axis_a=axis, axis_b=axis,
                         kind=capi.JOINT_SLIDER if is_slider else capi.JOINT_HINGE))

        def more():
            return dict(compliance=rng.uniform(0.0, 0.01) if rng.uniform() < 0.5 else 0.0,
                        max_force=rng.uniform(0.5, 5.0) if rng.uniform() < 0.5 else INF)
        if rng.uniform() < 0.4:
            lo = rng.uniform(-0.2, 0.0)
            lims.append((k, capi.LIMIT_HINGE, lo, lo + rng.uniform(0.0, 0.2), ref, ref))
        if rng.uniform() < (0.5 if is_slider else 0.9):
            kind, target = ((capi.DRIVE_ANGLE, rng.uniform(-0.3, 0.3)) if rng.uniform() < 0.5 else
                            (capi.DRIVE_ANGULAR_VELOCITY, rng.uniform(-5.0, 5.0)))
            drvs.append(dict(joint=k, kind=kind, target=target, ref_a=ref, ref_b=ref, **more()))
        if is_slider:
            if rng.uniform() < 0.6:
                lo = rng.uniform(-0.05, 0.0)
                lims.append((k, capi.LIMIT_SLIDE, lo, lo + rng.uniform(0.0, 0.05)))
            if rng.uniform() < 0.8:
                kind, target = ((capi.DRIVE_POSITION, rng.uniform(-0.2, 0.2)) if rng.uniform() < 0.5 else
                                (capi.DRIVE_VELOCITY, rng.uniform(-2.0, 2.0)))
                drvs.append(dict(joint=k, kind=kind, target=target, **more()))
    lims = [lims[i] for i in rng.permutation(len(lims))]
    drvs = [drvs[i] for i in rng.permutation(len(drvs))]
    return np.array(bodies), jc.joints_of(rows), jc.limits_of(lims), dc.drives_of(drvs)


def against_the_contact_free_model(state, joints, lims, drvs, h, substeps):
    """tests/joint_drive_model.py stepped `substeps` times, each substep against this model from the same state.  Returns
    (largest normalised error of a checked body-substep, extra entries, clamped entries, excluded, total body-substeps)."""
    shapes = pc.table()[1]
    sid = np.zeros(len(state), dtype=np.uint32)
    ext = np.maximum(pc.extents(sid, state), jc.arms({"sid": sid, "joints": joints}))
    pairs = [(int(j["body_a"]), int(j["body_b"])) for j in joints]
    worst, extras, clamped, left_out, total = 0.0, 0, 0, 0, 0
    for _ in range(substeps):
        got = jd.substep(state, joints, lims, drvs, h)
        res = pm.substep(state, shapes, sid, h, {}, joints=joints, limits=lims, drives=drvs)
        assert not res["n_points"].any() and not res["mask"][state[:, 0] > 0].any()
        e = pc.normalized_errors(got, res["state"], state, ext, h, pairs)
        x = dc.excluded(res)
        left_out, total = left_out + int(x.sum()), total + x.size
        worst = max(worst, np.where(x, 0, e).max())
        extras, clamped = extras + int(res["n_extra"].sum()), clamped + int(res["n_clamped"].sum())
        state = got
    return worst, extras, clamped, left_out, total


def test_the_contact_free_drive_model_lies_within_the_bound():
    """tests/joint_drive_model.py (f64, bodies that touch nothing) on 12 random scenes of 20 substeps, each substep against
    this model from the same state: within K_DRIVES, and the extras act."""
    worst, extras, clamped, left_out, total = 0.0, 0, 0, 0, 0
    for seed in range(12):
        state, joints, lims, drvs = contact_free_scene(seed)
        w, e, c, x, n = against_the_contact_free_model(state, joints, lims, drvs, 1.0 / 1200.0, 20)
        worst, extras, clamped, left_out, total = max(worst, w), extras + e, clamped + c, left_out + x, total + n
    print("joint_drive_model against the model: %.1f, %d extra entries, %d of them clamped, %d of %d body-substeps excluded" % (
        worst, extras, clamped, left_out, total))
    assert worst <= dc.K_DRIVES and extras > 2000 and clamped > 100 and left_out <= 0.10 * total


@pytest.mark.parametrize("name", ["wheel", "spring", "incline", "incline_stop", "lift_weak", "lift_strong", "prismatic"])
def test_the_known_answer_scenes_lie_within_the_bound(name):
    """The known-answer scenes of tests/joint_drive_model.py (a static base and a unit-mass body, anchors at the centres),
    eight substeps each from the scene's start, and eight more from where 40 substeps of that model have taken it."""
    rows, joints, lims, drvs, _, substeps, dt = jd.scene(name)
    h = dt / substeps
    worst, extras, _, left_out, _ = against_the_contact_free_model(rows, joints, lims, drvs, h, 8)
    for _ in range(40):
        rows = jd.substep(rows, joints, lims, drvs, h)
    later, more, _, left_out_later, _ = against_the_contact_free_model(rows, joints, lims, drvs, h, 8)
    print("%s: joint_drive_model against the model %.1f, then %.1f; excluded %d, then %d of 16 body-substeps" % (
        name, worst, later, left_out, left_out_later))
    assert max(worst, later) <= dc.K_DRIVES and left_out <= 3
    assert extras + more > 0 or name == "prismatic"    # (a slider that stays exactly on its axis has no extra entry at all)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_longdouble_model_equals_mpmath_model(name):
    """The substep that holds the scene's largest error, stage S on the longdouble model's manifolds, in longdouble and in
    40-digit mpmath (atan2 included): the states agree 2^11 times inside K_DRIVES and within a tenth of that maximum, and
    every limit, SLIDE limit and drive takes the same side of its decision: longdouble's rounding does not set the bound."""
    fast, ref = xm.native(), xm.mp(40)
    t = dc.trajectory(name)
    errs, excl, _ = dc.check_states(name, [fr[1] for fr in t["frames"]])
    worst = int(np.argmax([np.where(x, 0, e).max() for e, x in zip(errs, excl)]))
    start, _, res, _ = t["frames"][worst]
    given = {key: m for key, m in res["manifolds"].items() if m["p_ref"]}
    exact = {key: {"separated": False, "feature": m["feature"], "p_ref": [xm.lifted(ref, p) for p in m["p_ref"]],
                   "p_inc": [xm.lifted(ref, p) for p in m["p_inc"]]} for key, m in given.items()}
    a = dc.model(name, start, num=fast, manifolds=given)
    b = dc.model(name, start, num=ref, manifolds=exact)
    assert [(k, kind, err == 0) for k, kind, _, err in a["limits"]] == [(k, kind, err == 0) for k, kind, _, err in b["limits"]]
    assert [(k, e == 0) for k, _, e in a["slides"]] == [(k, e == 0) for k, _, e in b["slides"]]
    assert [(i, e == 0, c) for i, _, e, c, _ in a["drives"]] == [(i, e == 0, c) for i, _, e, c, _ in b["drives"]]
    for key in ("n_joint", "n_extra", "n_clamped", "mask"):
        assert np.array_equal(a[key], b[key]), key
    d = np.abs(ref.to_f64(xm.lifted(ref, a["state"]) - b["state"]))
    scale = pc.scales(start, fast.to_f64(a["state"]), t["ext"], xk.joint_links(t, res))
    turn = scale / t["ext"]
    h = t["h"]
    e = np.max(np.stack([d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * turn),
                         d[:, 22:25].max(axis=1) * h / (pc.EPS * scale), d[:, 25:28].max(axis=1) * h / (pc.EPS * turn)]), axis=0)
    top = xk.worst(errs, excl)
    print("%s substep %d: longdouble against mpmath %.4f = %.2g of the bound; the scene's maximum %.1f" % (
        name, worst, e.max(), e.max() / dc.K_DRIVES, top))
    assert e.max() <= dc.K_DRIVES / 2 ** 11 and e.max() <= 0.1 * top


# The scene on which each wrong reading of the MODEL leaves the bound, and the measured factor (worst error / K_DRIVES).
CAUGHT_BY = {"slider_keeps_positional": ("ends-h240", 9.1e11), "perpendicular_sign_a": ("ends-h240", 1.9e12),
             "extras_uncounted": ("ends-h240", 1.7e12), "nonbinding_slide_counted": ("lifts-h240", 1.0e9),
             "drive_without_base_compliance": ("wheels-h1200", 6.1e9), "clamp_by_h": ("wheels-h240", 2.4e9),
             "clamped_uncounted": ("lifts-h240", 1.2e9), "velocity_from_integrated": ("lifts-h240", 2.4e8),
             "extras_from_integrated": ("lifts-h240", 7.6e8), "wrap_dropped": ("wheels-h240", 1.3e12),
             "angular_drive_same_sign": ("wheels-h240", 6.1e10), "linear_drive_w_without_angular": ("ends-h240", 5.7e8)}


@pytest.mark.parametrize("mutation", pm.DRIVE_MUTATIONS)
def test_the_bound_sees_each_misreading(mutation):
    """Each wrong variant of the model pushes the f64 evaluation beyond K_DRIVES on the named scene, on a body-substep that
    the true model checks."""
    name, factor = CAUGHT_BY[mutation]
    t = dc.trajectory(name)
    worst = 0.0
    for start, want, res, _ in t["frames"]:
        wrong = dc.model(name, start, mutation=mutation, manifolds=res["manifolds"])
        worst = max(worst, np.where(dc.excluded(res), 0.0, dc.errors(name, want, wrong, start)).max())
    print("%s on %s: %.3g x the bound (recorded: %.2g)" % (mutation, name, worst / dc.K_DRIVES, factor))
    assert worst > dc.K_DRIVES


@pytest.mark.parametrize("name", ["lifts-h1200", "wheels-h1200"])
@pytest.mark.parametrize("without", ["drives", "slide limits"])
def test_the_bound_sees_the_extras(name, without):
    """The model without the drives, and without the SLIDE limits, leaves the bound of the full model on scenes (a) and (b):
    the device control of test_gpu_xprec_drives.py, on the CPU reading."""
    t = dc.trajectory(name)
    start, want, res, _ = t["frames"][0]
    less = dc.model(name, start, num=xm.f64(), without=(without,))
    e = np.where(dc.excluded(res), 0, dc.errors(name, xm.f64().to_f64(less["state"]), res, start)).max()
    assert e > dc.K_DRIVES


# ---- invariants of the model itself -----------------------------------------------------------------------------------
DRIVEN = {"position": (capi.JOINT_SLIDER, capi.DRIVE_POSITION, 0.05), "velocity": (capi.JOINT_SLIDER, capi.DRIVE_VELOCITY, 1.5),
          "angle": (capi.JOINT_HINGE, capi.DRIVE_ANGLE, 0.2), "angular-velocity": (capi.JOINT_HINGE, capi.DRIVE_ANGULAR_VELOCITY, 3.0),
          "prismatic": (capi.JOINT_SLIDER, capi.DRIVE_ANGULAR_VELOCITY, -2.0)}


def free_driven_pair(seed, which, anchor_error):
    """Two cubes 3 m apart, far from the ground, tilted, no forces: a slider or hinge whose axes are one world direction
    (aligned to rounding), with one drive of max_force = inf; `prismatic` adds a POSITION drive and a binding SLIDE limit."""
    rng = np.random.default_rng(seed)
    bodies = np.array([pc.new_body(pc.CUBE, (0.0, 0.0, 8.0), jc.tilt(rng, 0.4), gravity=False),
                       pc.new_body(pc.CUBE, (3.0, 0.5, 8.2), jc.tilt(rng, 0.4), gravity=False)])
    kind, drive_kind, target = DRIVEN[which]
    make = dc.slider if kind == capi.JOINT_SLIDER else dc.hinge
    row = make(bodies, 0, 1, np.array([2.0, 0.7, 8.6]), (0.3, -0.5, 0.8), anchor_error)
    drvs = [dict(joint=0, kind=drive_kind, target=target, **(dc.refs(bodies, row, 0.1) if drive_kind in dc.ANGULAR else {}))]
    lims = []
    if which == "prismatic":
        drvs.append(dict(joint=0, kind=capi.DRIVE_POSITION, target=0.03, compliance=0.002))
        lims.append((0, capi.LIMIT_SLIDE, dc.travel(bodies, row) + 0.01, 1.0))
    return bodies, jc.joints_of([row]), jc.limits_of(lims), dc.drives_of(drvs)


@pytest.mark.parametrize("which", list(DRIVEN))
def test_model_conserves_momentum_on_a_free_driven_pair(which):
    """No gravity, no contact, max_force = inf.  Every extra entry is +-lambda n at p_a, p_b or +-lambda n about one axis, so
    sum m dx vanishes to rounding.  Angular momentum: the angular kinds are a pure couple; a linear entry along n acts at two
    points d = r + s n apart and leaves the moment lambda r x n, first order in the perpendicular offset |r| (2e-3 m here,
    against the 2e-2 that test_xprec_joints_oracle.py allows the second-order rest of a turn).  The perpendicular_sign_a
    and angular_drive_same_sign readings leave all of the moved momentum."""
    num = xm.native()
    bodies, joints, lims, drvs = free_driven_pair(3, which, (0.001, -0.001, 0.0015))
    sid = np.zeros(2, dtype=np.uint32)
    res = pm.substep(bodies, pc.table()[1], sid, pc.HS[1], {}, joints=joints, limits=lims, drives=drvs)
    assert res["n_extra"].min() >= (3 if which == "prismatic" else 1) and not res["n_points"].any() and not res["n_clamped"].any()
    before = num.conv(bodies)
    lin, ang = xk.momenta(num, before, res["state"], bodies)
    moved = np.abs(num.to_f64(res["state"][:, 31:38] - before[:, 31:38])).max() / bodies[:, 0].min()
    assert moved > 1e-4
    assert np.abs(lin).max() <= max(1e-15 * moved, 8 * 9.0 * 2.0 ** -63), (lin, moved)      # or a few ulps of the model at 9 m
    assert np.abs(ang).max() <= 2e-2 * moved, (ang, moved)
    wrong = "angular_drive_same_sign" if which in ("angle", "angular-velocity") else "perpendicular_sign_a"
    bad = pm.substep(bodies, pc.table()[1], sid, pc.HS[1], {}, joints=joints, limits=lims, drives=drvs, mutation=wrong)
    lin, ang = xk.momenta(num, before, bad["state"], bodies)
    assert max(np.abs(lin).max(), np.abs(ang).max()) > 0.1 * moved


@pytest.mark.parametrize("which", list(DRIVEN))
def test_model_mirrors_when_a_and_b_are_swapped(which):
    """The joint written from b's side -- bodies, anchors, axes and refs swapped; s and phi change sign, so the targets do
    and the SLIDE bounds swap with their signs -- moves both bodies as before, to the rounding of the two axes' alignment.  (s
    and phi are measured along a's axis: the mirror image is exact only while a_w == b_w, so the bodies spin about it alone.)"""
    num = xm.native()
    bodies, joints, lims, drvs = free_driven_pair(5, which, (0.004, -0.003, 0.002))
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    bodies[:, 25:28] = [axis * 2.0, axis * -1.5]                         # spins about the axis: the axes stay aligned
    bodies[:, 22:25] = [[0.2, 0.1, -0.3], [-0.1, 0.4, 0.2]]
    swapped, mirrored, turned = joints.copy(), lims.copy(), drvs.copy()
    for x, y in (("body_a", "body_b"), ("anchor_a", "anchor_b"), ("axis_a", "axis_b")):
        swapped[x], swapped[y] = joints[y], joints[x]
    turned["ref_a"], turned["ref_b"], turned["target"] = drvs["ref_b"], drvs["ref_a"], -drvs["target"]
    mirrored["lower"], mirrored["upper"] = -lims["upper"], -lims["lower"]
    sid = np.zeros(2, dtype=np.uint32)
    one = pm.substep(bodies, pc.table()[1], sid, pc.HS[1], {}, joints=joints, limits=lims, drives=drvs)
    two = pm.substep(bodies, pc.table()[1], sid, pc.HS[1], {}, joints=swapped, limits=mirrored, drives=turned)
    assert np.array_equal(one["n_joint"], two["n_joint"]) and np.array_equal(one["n_extra"], two["n_extra"])
    assert one["n_extra"].min() >= (3 if which == "prismatic" else 1)
    d = np.abs(num.to_f64(one["state"] - two["state"]))
    assert d[:, 31:38].max() <= 1e-14 and d[:, 22:28].max() <= 1e-14 / pc.HS[1], d.max()
