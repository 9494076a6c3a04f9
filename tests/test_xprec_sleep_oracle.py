"""Awake bodies in contact with sleepers (include/xpbd.h, "SLEEPING", rules (a)-(c)): the f64 evaluation of the model against the
extended-precision model (xprec_pairs_model.substep with asleep=), frame by frame; the 40-digit model on the frames that hold the
maxima; the exact scene's answers by name; a mutation table; the caps and floors of the scene set; frames of S = 2 and 3
substeps chained with the sleepers frozen; and mechanics of the model itself.  Scenes, bound and exclusions: xprec_sleep_cases.py;
the measured figures: DESIGN 1g."""
import numpy as np
import pytest

import xprec_bounce_cases as bc
import xprec_check as xk
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
import xprec_sleep_cases as sc
from golden_util import bits_equal

SCENE_NAMES = list(sc.SCENES)
CHAIN_FRAMES = 4
SEEDED_VELOCITY, SEEDED_SPIN = (0.5, -0.3, 0.2), (0.2, 0.1, -0.4)


def f64_states(name):
    return [fr[1] for fr in sc.trajectory(name)["frames"]]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_f64_reading_against_the_model_frame_by_frame(name):
    """Every checked body-substep of the f64 evaluation of the model is within bounds() of the longdouble model; the exclusion caps
    and the floor hold over all body-substeps and over those with a sleeper's point; a sleeper's state is its input to the bit;
    the scene holds what its description says; the exact scene does what the header says, case by case."""
    t = sc.trajectory(name)
    errs, excl, entry = sc.check_states(name, f64_states(name))
    x, c = np.concatenate(excl), np.concatenate(entry)
    print("%s: f64 evaluation %.1f; excluded %d of %d body-substeps, %d of %d with a sleeper's point" % (
        name, xk.worst(errs, excl), x.sum(), x.size, (x & c).sum(), c.sum()))
    xk.assert_caps(name, excl, entry, floor=sc.caps_floor(name))
    native = xm.native()
    for f, (start, want, res, s) in enumerate(t["frames"]):
        z = s["asleep"]
        assert len(start) <= 40 and not np.isnan(want).any() and z.any()
        assert bits_equal(want[z], start[z]) and bits_equal(native.to_f64(res["state"])[z], start[z])     # rule (b)
        assert not res["mask"][z].any() and not res["n_points"][z].any()
        assert not any(pm.is_fixed(xm._unpack(start, native))[list(k)].all() or z[list(k)].all() for k in res["manifolds"])   # rule (a)
        moved = (want[:, 31:38] != start[:, 31:38]).any(axis=1)
        assert moved[sc.carries(res)].all()
        if name.startswith(("general", "materials", "bouncing-h", "damped")):
            assert tuple(start[0, 28:31]) == sc.COM and z[0] and len(set(np.diag(start[0, 1:10].reshape(3, 3)))) == 3
            assert {pc.HULL16, pc.HULL18} <= set(s["sid"][z].tolist()) and set(range(5)) <= set(s["sid"][s["probes"]].tolist())
            assert len(set(start[:, 0].tolist())) >= 6                   # unequal masses
        if name.startswith(("stack", "bouncing-stack")):
            assert (s["labels"][z] == "stack").all() and z.sum() == 9
        if name.startswith("materials"):
            assert len(set(s["mu"].tolist())) == len(pc.MUS) and s["speed"] == (3.0 if "3" in name.split("-")[0] else 0.0)
        if name.startswith("bouncing"):
            assert set(s["e"][z].tolist()) >= {0.4, 0.8} or name.startswith("bouncing-stack")
            assert (s["e"][z] > 0).any() and (s["e"][~z] > 0).any()
        if name.startswith("damped"):
            rows = s["rows"]
            assert (rows["linear"][z] > 0).any() and np.isfinite(rows["max_linear_speed"][z]).any()
            assert (rows["linear"][~z] > 0).any() and np.isfinite(rows["max_linear_speed"][~z]).any()
    if name.startswith("shared"):
        assert sum(int((sc.carries(r) & (r["mask"] != 0) & (r["n_points"] > r["n_sleeper_points"])).sum()) for _, _, r, _ in t["frames"]) >= 8


def test_the_exact_scene_by_name():
    """EQUAL and HEAVY: the probe's displacement is, to the bit, its own part of the all-awake substep's -- in which the sleeper
    moves by exactly minus that (equal masses: each takes half of what closes) or by minus that / 1024 -- and nothing else of it
    changes.  TOUCH: SAT value 0 is no contact, and the probe has the lone box's bits."""
    f64 = xm.f64()
    for f, (start, want, res, s) in enumerate(sc.trajectory("exact-h1024")["frames"]):
        awake = f64.to_f64(sc.evaluate(s, num=f64, asleep=None)["state"])
        for (sleeper, probe), ratio in ((sc.EXACT_EQUAL, 1.0), (sc.EXACT_HEAVY, 1024.0)):
            dz = want[probe, 33] - start[probe, 33]
            assert dz > 0 and res["n_sleeper_points"][probe] == 4 and res["n_points"][probe] == 4
            assert bits_equal(want[probe], awake[probe])
            # (the awake twin's position is rounded once more, to the spacing of doubles at 8 m, when the small step is added)
            assert abs(awake[sleeper, 33] - start[sleeper, 33] + dz / ratio) <= (0.0 if ratio == 1.0 else np.spacing(8.0) / 2)
            assert bits_equal(want[sleeper], start[sleeper])
            assert bits_equal(want[probe, 34:38], start[probe, 34:38]) and bits_equal(want[probe, 31:33], start[probe, 31:33])
        # the whole correction of a fixed body would be more than the share: the sleeper is not a fixed body
        fixed = f64.to_f64(sc.evaluate(s, num=f64, mutation="sleeper_fixed")["state"])
        equal = sc.EXACT_EQUAL[1]
        assert fixed[equal, 33] - start[equal, 33] > 1.5 * (want[equal, 33] - start[equal, 33])
        sleeper, probe = sc.EXACT_TOUCH
        assert (sleeper, probe) not in res["manifolds"] and res["n_points"][probe] == 0
        lone = want[sc.EXACT_LONE].copy()
        assert lone[31] - want[probe, 31] == sc.EXACT_LONE_SHIFT
        lone[31] = want[probe, 31]
        assert bits_equal(want[probe], lone)
        alone = f64.to_f64(sc.evaluate(dict(s, sid=s["sid"][1:], e=None, mu=None, rows=None), state=start[1:], num=f64,
                                       asleep=s["asleep"][1:])["state"])
        assert bits_equal(alone[probe - 1], want[probe])


def maxima(name):
    a = b = 0.0
    for f, (start, want, res, s) in enumerate(sc.trajectory(name)["frames"]):
        e = np.where(sc.excluded(res, s), 0, sc.errors(s, want, res))
        a, b = max(a, e[bc.one_point(res)].max(initial=0.0)), max(b, e[~bc.one_point(res)].max(initial=0.0))
    return a, b


def test_the_measured_maxima_fit_eight_times_under_the_existing_bounds():
    """8x the largest error of a checked body-substep fits under the bounds as they stand: under K_BOUNCE on a body with a
    one-point stage-6 entry, under K_PLAIN on every other one (xprec_bounce_cases.bounds(), which check_states applies), and on
    the scenes without restitution under K_PAIRS as well.  No new single-substep bound is introduced."""
    with_one = others = plain = 0.0
    for name in SCENE_NAMES:
        a, b = maxima(name)
        print("%s: %.1f with a one-point entry, %.1f without" % (name, a, b))
        with_one, others = max(with_one, a), max(others, b)
        if not sc.is_bouncing(name):
            assert a == 0.0
            plain = max(plain, b)
    print("largest normalised errors: %.1f (8x = %.0f, K_BOUNCE = %g), %.1f without a one-point entry (8x = %.0f, K_PLAIN = %g), "
          "%.1f without restitution (8x = %.0f, K_PAIRS = %g)" % (with_one, 8 * with_one, bc.K_BOUNCE, others, 8 * others, bc.K_PLAIN,
                                                                plain, 8 * plain, pc.K_PAIRS))
    assert 8 * with_one <= bc.K_BOUNCE and 8 * others <= bc.K_PLAIN and 8 * plain <= pc.K_PAIRS


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_longdouble_model_equals_mpmath_model(name):
    """The frame that holds the scene's largest error, on the longdouble model's manifolds, in longdouble and in 40-digit mpmath:
    the states agree 2^11 times inside the bound and within a tenth of that maximum, with the same sleeper points and entries."""
    fast, ref = xm.native(), xm.mp(40)
    t = sc.trajectory(name)
    errs, excl, _ = sc.check_states(name, f64_states(name))
    per_frame = [float(np.where(x, 0, e).max()) for e, x in zip(errs, excl)]
    f = int(np.argmax(per_frame))
    start, _, res, s = t["frames"][f]
    given = {key: m for key, m in res["manifolds"].items() if m["p_ref"]}
    exact = {key: {"separated": False, "feature": m["feature"], "p_ref": [xm.lifted(ref, p) for p in m["p_ref"]],
                   "p_inc": [xm.lifted(ref, p) for p in m["p_inc"]], **({"normal": xm.lifted(ref, m["normal"])} if "normal" in m else {})}
             for key, m in given.items()}
    a = sc.evaluate(s, num=fast, manifolds=given)
    b = sc.evaluate(s, num=ref, manifolds=exact)
    for key in ("mask", "n_points", "n_sleeper_points", "bounce_pair_entries", "bounce_ground_entries", "cap_fired_linear",
                "cap_fired_angular"):
        if key in a:
            assert np.array_equal(a[key], b[key]), key
    d = np.abs(ref.to_f64(xm.lifted(ref, a["state"]) - b["state"]))
    scale = pc.scales(start, fast.to_f64(a["state"]), s["ext"], list(res["manifolds"]))
    turn = scale / s["ext"]
    h = s["h"]
    e = np.max(np.stack([d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * turn),
                         d[:, 22:25].max(axis=1) * h / (pc.EPS * scale), d[:, 25:28].max(axis=1) * h / (pc.EPS * turn)]), axis=0)
    print("%s frame %d: longdouble against mpmath %.4f = %.2g of K_PLAIN; the scene's maximum %.1f" % (
        name, f, e.max(), e.max() / bc.K_PLAIN, per_frame[f]))
    assert e.max() <= bc.K_PLAIN / 2 ** 11 and e.max() <= max(0.1 * per_frame[f], 0.05)


# ---- the mutation table -----------------------------------------------------------------------------------------------------------
# The scene on which the f64 evaluation of each wrong reading of the MODEL leaves the bound of the true longdouble model, and the
# measured factor (worst error / the body's bound).
# "seeded": the sleepers of the model's INPUT carry a velocity and a spin written by hand (SEEDED_*).  No device state has one:
# step 3 of the sleep pass stores +0.0 and every edit of a sleeper wakes it before the next step.  With +0.0 stored, stage 6
# reading the stored velocity reads the same zero, and a sleeper's drag row multiplies zero: both readings are invisible on every
# reachable scene (asserted below: not one bit of the f64 evaluation moves), and only the seeded input shows them.
CAUGHT_BY = {"sleeper_share_applied": ("general-h240", False, 3.1e10), "sleeper_fixed": ("general-h240", False, 2.2e10),
             "record_from_integrated": ("general-h240", False, 5.4e8), "record_after_ground": ("general-h240", False, 7.0e4),
             "record_without_com": ("general-h240", False, 1.1e12),
             "stage6_reads_stored_velocity": ("bouncing-h240", True, 1.4e10), "sleeper_point_twice": ("general-h240", False, 5.5e10),
             "sleeper_point_uncounted": ("general-h240", False, 1.6e11), "sleeper_drag_applied": ("damped-h240", True, 8.2e8)}
INVISIBLE_UNSEEDED = {"stage6_reads_stored_velocity": "bouncing-h240", "sleeper_drag_applied": "damped-h240"}
STALE_SECOND_RECORD = ("general-h240", 1.5e9)


def seeded(s):
    start = s["bodies"].copy()
    start[s["asleep"], 22:25], start[s["asleep"], 25:28] = SEEDED_VELOCITY, SEEDED_SPIN
    return start


def factor_of(name, mutation, seed):
    worst = 0.0
    for f, (start, want, res, s) in enumerate(sc.trajectory(name)["frames"]):
        if seed:
            start = seeded(s)
            want = xm.f64().to_f64(sc.evaluate(s, state=start, num=xm.f64())["state"])
            res = sc.frame_result(s, start, f)
            assert bits_equal(want[s["asleep"]], start[s["asleep"]])     # the true reading keeps the seeded bits and reads zero
        # a record's frame acts through stage N alone (P0 = P1 leaves a sleeper's point no travel, whatever the frame is): the
        # readings of the record run their own stage N, the others the model's manifolds
        wrong = sc.evaluate(s, state=start, num=xm.f64(), mutation=mutation, manifolds=None if mutation.startswith("record") else res["manifolds"])
        worst = max(worst, np.where(sc.excluded(res, s), 0.0, sc.errors(s, xm.f64().to_f64(wrong["state"]), res, start) / sc.bounds(res)).max())
    return worst


@pytest.mark.parametrize("mutation", list(CAUGHT_BY))
def test_the_bound_sees_each_misreading(mutation):
    """Each wrong variant of the model pushes the f64 evaluation beyond the bound on the named scene, on a body-substep that the
    true model checks."""
    name, seed, recorded = CAUGHT_BY[mutation]
    worst = factor_of(name, mutation, seed)
    print("%s on %s%s: %.3g x the bound (recorded: %.2g)" % (mutation, name, " (seeded)" if seed else "", worst, recorded))
    assert worst > 1.0


@pytest.mark.parametrize("mutation", list(INVISIBLE_UNSEEDED))
def test_two_readings_are_invisible_on_every_reachable_state(mutation):
    name = INVISIBLE_UNSEEDED[mutation]
    for f, (start, want, res, s) in enumerate(sc.trajectory(name)["frames"][:3]):
        wrong = xm.f64().to_f64(sc.evaluate(s, num=xm.f64(), mutation=mutation)["state"])
        assert bits_equal(np.abs(wrong), np.abs(want)), (mutation, f)    # (a sleeper's -0.0 from 0 * k aside)


def test_every_listed_misreading_has_a_row():
    assert set(CAUGHT_BY) == set(pm.SLEEP_MUTATIONS)


def test_without_the_asleep_set_the_model_leaves_the_bound():
    """The control of the device module on the CPU reading: everybody awake from the same state."""
    name = "general-h1200"
    worst = 0.0
    for f, (start, want, res, s) in enumerate(sc.trajectory(name)["frames"][:2]):
        awake = xm.f64().to_f64(sc.evaluate(s, num=xm.f64(), asleep=None)["state"])
        worst = max(worst, np.where(sc.excluded(res, s), 0, sc.errors(s, awake, res) / sc.bounds(res)).max())
    print("%s with everybody awake: %.3g x the bound" % (name, worst))
    assert worst > 1.0


@pytest.mark.parametrize("name", ["general-h240", "exact-h1024"])
def test_gjk_manifolds_from_the_models_frames_cover_half_of_the_touching_bodies(name):
    """What the device module holds GJK + EPA to: the helper reproduces the manifolds of at least half of the touching
    body-substeps from the model's frames, the f64 evaluation on them stays within K_PAIRS, and no pair has two inert ends."""
    checked = total = 0
    for f in range(sc.FRAMES):
        s = sc.build(name, f)
        res, x, touching = sc.gjk_result(s, s["bodies"])
        want = xm.f64().to_f64(sc.evaluate(s, num=xm.f64(), manifolds=res["manifolds"])["state"])
        e = sc.errors(s, want, res)
        assert (e[~x] <= pc.K_PAIRS).all() and bits_equal(want[s["asleep"]], s["bodies"][s["asleep"]])
        assert not any(s["asleep"][list(k)].all() for k in res["manifolds"])
        checked, total = checked + int((touching & ~x).sum()), total + int(touching.sum())
    print("%s: %d of %d touching body-substeps on reproducible GJK + EPA manifolds" % (name, checked, total))
    assert checked >= 0.5 * total and total >= 30


# ---- frames of S substeps -------------------------------------------------------------------------------------------------------
def chain_figures(name, substeps, mutation_at=None):
    """(normalised errors, excluded, carries) of the f64 chain against the longdouble chain, lists over frames."""
    errs, excl, entry = [], [], []
    for f in range(CHAIN_FRAMES):
        s = sc.build(name, f)
        res, x, c, links = sc.chain(s, s["bodies"], substeps)
        got, _, _, _ = sc.chain(s, s["bodies"], substeps, num=xm.f64(), mutation_at=mutation_at)
        e = sc.chain_errors(s, xm.f64().to_f64(got["state"]), res, s["bodies"], links, substeps)
        errs.append(e), excl.append(x), entry.append(c)
    return errs, excl, entry


@pytest.mark.parametrize("substeps", sc.CHAIN_SUBSTEPS)
def test_the_f64_chain_stays_within_the_recorded_chain_bound(substeps):
    """Scenes (a), (c) and (e), the first CHAIN_FRAMES frames as one frame of S substeps: the f64 evaluation chained S times against
    the longdouble model chained S times, the sleepers frozen.  K_SLEEP_CHAIN[S] is 8x the largest figure printed here, over the
    chained scenes; it is measured against the model only."""
    largest = 0.0
    for name in sc.CHAINED:
        errs, excl, entry = chain_figures(name, substeps)
        e = xk.worst(errs, excl)
        x, c = np.concatenate(excl), np.concatenate(entry)
        print("%s, S = %d: f64 chain against the longdouble chain %.1f; excluded %d of %d, %d of %d with a sleeper's point" % (
            name, substeps, e, x.sum(), x.size, (x & c).sum(), c.sum()))
        xk.assert_caps(name, excl, entry)
        largest = max(largest, e)
    print("S = %d: largest %.2f, 8x = %.1f, K_SLEEP_CHAIN = %g" % (substeps, largest, 8 * largest, sc.K_SLEEP_CHAIN[substeps]))
    assert 8 * largest <= sc.K_SLEEP_CHAIN[substeps] <= 8.5 * largest


def test_a_stale_second_record_set_leaves_the_chain_bound():
    """S = 2: the second substep reads the sleeper's record from a pose integrated once -- what a second record set that was
    never rewritten looks like.  Invisible at S = 1 by construction."""
    name, recorded = STALE_SECOND_RECORD
    errs, excl, _ = chain_figures(name, 2, mutation_at={1: "record_from_integrated"})
    worst = xk.worst(errs, excl) / sc.K_SLEEP_CHAIN[2]
    print("a stale second record set on %s, S = 2: %.3g x K_SLEEP_CHAIN (recorded: %.2g)" % (name, worst, recorded))
    assert worst > 1.0


# ---- mechanics of the model itself ------------------------------------------------------------------------------------------------
def test_the_awake_bodys_correction_is_its_own_part_of_the_all_awake_substep():
    """Both at rest, no external force: the probe's result with the sleeper asleep equals, to rounding, its result when the
    sleeper is awake and takes its share -- the record is the sleeper's own pose, mass and inertia, and only its share is
    dropped.  Pairs of scene (a), frame 0, each pair alone, pushed 1 cm into each other."""
    s = sc.build("general-h240", 0)
    num = xm.native()
    z = np.nonzero(s["asleep"])[0]
    checked = 0
    for sleeper in z:
        probe = sleeper + 1
        pair = s["bodies"][[sleeper, probe]].copy()
        pair[:, 10:28] = 0.0
        pair[:, 33] += 10.0                                              # clear of the ground: the awake twin has no other contact
        pc.touch(pair[0], s["sid"][sleeper], pair[1], s["sid"][probe], pair[1, 31:34] - pair[0, 31:34], 0.01)
        kw = dict(h=s["h"], num=num)
        asleep = pm.substep(pair, pc.table()[1], s["sid"][[sleeper, probe]], asleep=np.array([True, False]), **kw)
        awake = pm.substep(pair, pc.table()[1], s["sid"][[sleeper, probe]], **kw)
        assert asleep["n_sleeper_points"][1] >= 1
        d = np.abs(num.to_f64(asleep["state"][1] - awake["state"][1]))
        moved = np.abs(num.to_f64(asleep["state"][1, 31:38]) - pair[1, 31:38]).max()
        # rounding: the awake twin's integrate renormalises its rotation, an f64 quaternion whose length is 1 to 2^-53 only, so
        # its surface moves by that much of its extent; 16 x 2^-53 against a correction of millimetres
        assert moved > 1e-5 and d[31:38].max() <= 16 * pc.EPS, (sleeper, d[31:38].max())
        assert np.abs(num.to_f64(awake["state"][0, 31:38]) - pair[0, 31:38]).max() > 1e-6       # and the awake twin did take it
        assert bits_equal(num.to_f64(asleep["state"][0]), pair[0])
        checked += 1
    assert checked == 8


def test_a_sleepers_returned_state_and_mask_are_the_input():
    s = sc.build("shared-h240", 0)
    start = seeded(s)
    mask = np.arange(len(start), dtype=np.uint32) + 5
    for num in (xm.native(), xm.f64()):
        res = sc.evaluate(s, state=start, num=num, contact_mask=mask)
        z = s["asleep"]
        assert bits_equal(num.to_f64(res["state"])[z], start[z]) and np.array_equal(res["mask"][z], mask[z])
        assert not np.array_equal(res["mask"][~z], mask[~z])
    plain = sc.evaluate(s, num=xm.f64(), asleep=np.zeros(len(start), dtype=bool))
    same = sc.evaluate(s, num=xm.f64(), asleep=None)
    assert bits_equal(xm.f64().to_f64(plain["state"]), xm.f64().to_f64(same["state"]))           # an empty set is no set
