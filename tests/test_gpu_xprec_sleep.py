"""The scenes of tests/xprec_sleep_cases.py through the C ABI (World.set_sleeping with set_materials, set_restitution, set_damping,
set_max_depenetration_speed; SAT): an awake body in contact with a sleeper within the bound of the extended-precision model
(xprec_pairs_model.substep with asleep=, include/xpbd.h "SLEEPING" rules (a)-(c)) on every scene and under the fused, the unfused
and the restitution schedule of the step; every sleeper bit-frozen across the frame; frames of S = 2 and 3 substeps against the
model chained S times; the schedules' bits against one another at S = 1, 2, 3 and 20; the one-lane-per-body path behind a far
field; scenes (a) and (g) under GJK + EPA on the manifolds the model can reproduce; and the control world in which nobody sleeps.

How a world reaches "a sleeper under an awake body" (nothing puts a body to sleep by request): the sleepers-to-be are uploaded at
rest and the probes parked far away, each alone, faster than the thresholds; one step with frames_to_sleep = 1 puts exactly the
intended bodies to sleep; the download then holds the sleepers' bits as the device left them, and the model is seeded from it;
set_dynamics on the probes alone -- naming an awake body wakes nobody -- moves them into place; then the frame under test."""
import numpy as np
import pytest

import islands_model as im
import xprec_check as xk
import xprec_device as xd
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_sleep_cases as sc
from constraint_solver_amd import capi
from golden_util import bits_equal
from sleep_common import DYN

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(sc.SCENES)
# natural: the scene's own settings (the fused schedule unless the scene bounces or is damped); kinematic: a VELOCITY entry of zero
# on a far static box, which selects the unfused schedule and moves nothing; restitution: a coefficient on that far box, which
# touches nothing, so the velocity pass runs over everybody, makes no entry of its own and puts the sleepers back
SCHEDULES = ("natural", "kinematic", "restitution")
# What puts the sleepers-to-be to sleep: linear and angular speed at rest, frames_to_sleep.  The linear speed lies below the
# smallest cap of scene (f), which a parked probe keeps, and above what a step leaves a sleeper-to-be with (0.3 m/s at most: a
# stack 2^-12 m deep in itself at h = 1/1200); a parked probe does not spin, so the angular speed only has to admit the
# sleepers-to-be (the small tetrahedron pushed out of the ground turns at more than 0.4 rad/s).
THRESHOLDS = (0.4, 50.0, 1)
# The configuration of the frame under test (set_sleeping on a world that sleeps replaces the configuration and keeps the state):
# the pass at its end must not put the woken group and its probe to sleep again, which would zero the probe's velocities.
STRICT = (1e-6, 1e-6, 1000)
PARK_SPEED = 100.0
CHAIN_FRAMES = 4
_MODEL = {}


def reach(w, s, schedule="natural", far=0, sleeping=True):
    """Uploads, sleeps, downloads and moves the probes into place.  Returns the state at the start of the frame under test (the
    scene's bodies), the sleepers' contact masks and the sleep state (asleep, group) before that frame."""
    n = len(s["sid"])
    probes = np.nonzero(s["probes"])[0]
    parked = s["bodies"].copy()
    parked[probes, 31], parked[probes, 32], parked[probes, 33] = -500.0 - 50.0 * np.arange(len(probes)), -500.0, 300.0
    parked[probes, 22:25], parked[probes, 25:28] = (PARK_SPEED, 0.0, 0.0), 0.0
    post = pc.new_body(pc.CUBE, (-1000.0, 500.0, 50.0), static=True)
    extra, extra_sid = xd.far_field(far)
    m = 1 + len(extra)
    w.upload(np.concatenate([parked, post[None], extra]), np.concatenate([s["sid"], [pc.CUBE], extra_sid]).astype(np.uint32))
    w.set_contact_report(True)
    if sleeping:
        w.set_sleeping(*THRESHOLDS)
    if s["speed"]:
        w.set_max_depenetration_speed(s["speed"])
    if s["mu"] is not None:
        w.set_materials(np.concatenate([s["mu"], np.full(m, np.inf)]), s["ground_mu"])
    e = np.zeros(n + m) if s["e"] is None else np.concatenate([s["e"], np.zeros(m)])
    if schedule == "restitution":
        e[n] = 0.4
    if e.any() or s["ground_e"]:
        w.set_restitution(e, s["ground_e"], s["threshold"])
    if s["rows"] is not None:
        w.set_damping(np.concatenate([s["rows"], capi.body_damping(m)]))
    if schedule == "kinematic":
        w.set_kinematics(capi.kinematics([n], capi.KINEMATIC_VELOCITY, [(0.0, 0.0, 0.0)], [(0.0, 0.0, 0.0, 0.0)]))
    asleep = group = None
    if sleeping:
        w.step(s["h"], 1)
        asleep, _, group, _ = w.sleep_state()
        assert np.array_equal(asleep[:n].astype(bool), s["asleep"]), np.flatnonzero(asleep[:n].astype(bool) != s["asleep"])
        w.set_sleeping(*STRICT)
    rows = s["bodies"][probes]
    w.set_dynamics(probes, np.concatenate([rows[:, 31:38], rows[:, 22:28]], axis=1))
    if sleeping:
        again = w.sleep_state()[0]
        assert np.array_equal(again, asleep)                            # naming an awake body wakes nobody
    return w.download()[:n], im.masks_from_contacts(w.n, w.contacts())[:n], asleep, group


def model_of(name, f, s, start, substeps):
    """The longdouble model from the device's own start state; the same start under another schedule finds it again."""
    key = (name, f, substeps, start.tobytes())
    if key not in _MODEL:
        if substeps == 1:
            res = sc.frame_result(s, start, f)
            _MODEL[key] = (res, sc.excluded(res, s), sc.carries(res), list(res["manifolds"]))
        else:
            _MODEL[key] = sc.chain(s, start, substeps)
    return _MODEL[key]


def run(name, schedule="natural", substeps=1, far=0, frames=sc.FRAMES):
    """Every frame of the scene on the device: (start, state after the frame, model result, excluded, carries) per frame, with the
    sleepers' frozen bits, the asleep set before the frame and the wake after it asserted on the way."""
    out = []
    with xd.new_world() as w:
        for f in range(frames):
            s = sc.build(name, f)
            n = len(s["sid"])
            z = s["asleep"]
            start, masks, asleep, group = reach(w, s, schedule, far)
            if name.startswith(("stack", "bouncing-stack")):                # one group per stack, the slab its anchor
                stacks = group[:n][z].reshape(3, 3)
                assert (stacks == stacks[:, :1]).all() and len(set(stacks[:, 0].tolist())) == 3
            w.step(substeps * s["h"], substeps)
            got = w.download()[:n]
            after, _, _, counts = w.sleep_state()
            woken_by_pass = counts[2]
            assert bits_equal(got[z][:, DYN], start[z][:, DYN]) and bits_equal(got[z], start[z])             # rule (b)
            assert np.array_equal(im.masks_from_contacts(w.n, w.contacts())[:n][z], masks[z])
            assert not start[z, 22:28].any()
            res, x, c, links = model_of(name, f, s, start, substeps)
            if substeps == 1:
                # the header's wake step 1: the whole group of a touched sleeper wakes in this frame's pass
                touched = set()
                for i, j in res["manifolds"]:
                    m = res["manifolds"][(i, j)]
                    if m["p_ref"] and (i, j) not in res["undecided"] and z[i] != z[j] and m["margins"]["touch"] > 1e-7:
                        touched.add(int(group[i if z[i] else j]))
                assert touched and woken_by_pass >= sum(int((group[:n] == g).sum()) for g in touched), (f, woken_by_pass, touched)
                assert not any(after[:n][group[:n] == g].any() for g in touched) and counts[3] == 0
            out.append((start, got, res, x, c, links, s))
    return out


def verdict(name, frames, substeps=1):
    """The model's bound and the caps on this run; returns the largest normalised error of a checked body."""
    errs, excl, entry = xk.check_frames(
        name, [(start, res, dict(s, excluded=x, carries=c, links=links)) for start, _, res, x, c, links, s in frames],
        [fr[1] for fr in frames], excluded=lambda res, s: s["excluded"], carries=lambda res, s: s["carries"],
        errors=xk.scene_errors if substeps == 1 else lambda s, got, res, start: sc.chain_errors(s, got, res, start, s["links"], substeps),
        bound=sc.bounds if substeps == 1 else lambda res: sc.K_SLEEP_CHAIN[substeps])
    worst = xk.worst(errs, excl)
    print("%s, S = %d: device against the model %.1f" % (name, substeps, worst))
    return worst, excl, entry


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_awake_bodies_against_sleepers(name, schedule):
    frames = run(name, schedule)
    _, excl, entry = verdict(name, frames)
    xk.assert_caps(name, excl, entry, floor=sc.caps_floor(name))
    if schedule != "natural":                                                # the three schedules give one another's bits
        for a, b in zip(frames, run(name)):
            assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


def test_the_exact_scene_by_name_on_the_device():
    """EQUAL and HEAVY: to the bit the f64 evaluation, which is the probe's own part of the all-awake substep.  TOUCH: the lone
    box's bits."""
    for start, got, res, x, c, links, s in run("exact-h1024"):
        want = xm.f64().to_f64(sc.evaluate(s, state=start, num=xm.f64())["state"])
        for probe in (sc.EXACT_EQUAL[1], sc.EXACT_HEAVY[1]):
            assert got[probe, 33] > start[probe, 33] and bits_equal(got[probe], want[probe])
        probe = sc.EXACT_TOUCH[1]
        lone = got[sc.EXACT_LONE].copy()
        assert lone[31] - got[probe, 31] == sc.EXACT_LONE_SHIFT
        lone[31] = got[probe, 31]
        assert bits_equal(got[probe], lone) and bits_equal(got[probe], want[probe])


@pytest.mark.parametrize("substeps", sc.CHAIN_SUBSTEPS)
@pytest.mark.parametrize("name", sc.CHAINED)
def test_frames_of_several_substeps_against_the_chained_model(name, substeps):
    """One frame of S substeps -- the second record set of the fused schedule is read from the second substep on -- against the
    longdouble model chained S times with the sleepers frozen, within K_SLEEP_CHAIN[S] (measured on the CPU, f64 chain against
    longdouble chain); and the three schedules' bits."""
    frames = run(name, substeps=substeps, frames=CHAIN_FRAMES)
    _, excl, entry = verdict(name, frames, substeps)
    xk.assert_caps(name, excl, entry)
    for schedule in SCHEDULES[1:]:
        for a, b in zip(frames, run(name, schedule, substeps=substeps, frames=CHAIN_FRAMES)):
            assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), schedule


def test_twenty_substeps_on_the_stack_give_the_same_bits_under_every_schedule():
    runs = [run("stack-h240", schedule, substeps=20, frames=2) for schedule in SCHEDULES]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert bits_equal(a[1], b[1])
    start, got = runs[0][0][0], runs[0][0][1]
    assert np.abs(got - start)[:, 31:38].max() > 1e-4


@pytest.mark.parametrize("name", ["general-h1200", "stack-h240", "bouncing-h240"])
def test_behind_a_far_field_uses_one_lane_per_body(name):
    """Scenes (a), (c) and (e) with more than SMALL_WORLD bodies in the world: the same verdict, and the small world's bits."""
    frames = run(name, far=xd.SMALL_WORLD + 16, frames=CHAIN_FRAMES)
    _, excl, entry = verdict(name, frames)
    for a, b in zip(frames, run(name, frames=CHAIN_FRAMES)):
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["general-h1200", "general-h240", "exact-h1024"])
def test_gjk_epa_on_the_manifolds_the_model_can_reproduce(name):
    """Scenes (a) and (g) under GJK + EPA, where the narrowphase reads the sleepers' records: within K_PAIRS of stage S with asleep=
    on the manifolds xprec_pairs_cases' helper can reproduce from the model's frames (a face-aligned clip, or an EPA point whose
    depth and normal are stage N's), on at least half of the touching body-substeps; every sleeper bit-frozen."""
    checked = total = 0
    worst = 0.0
    with xd.new_world(narrowphase=capi.NARROWPHASE_GJK_EPA) as w:
        for f in range(sc.FRAMES):
            s = sc.build(name, f)
            n, z = len(s["sid"]), s["asleep"]
            start, masks, _, _ = reach(w, s)
            w.step(s["h"], 1)
            got = w.download()[:n]
            assert bits_equal(got[z], start[z]) and np.array_equal(im.masks_from_contacts(w.n, w.contacts())[:n][z], masks[z])
            res, x, touching = sc.gjk_result(s, start)
            e = sc.errors(s, got, res, start)
            bad = np.nonzero(~x & ~(e <= pc.K_PAIRS))[0]
            assert not len(bad), "%s GJK frame %d: bodies %s beyond K = %g: %s" % (name, f, bad[:8], pc.K_PAIRS, e[bad[:8]])
            worst = max(worst, float(np.where(x, 0, e).max()))
            carrying = touching & sc.carries(res)
            checked, total = checked + int((touching & ~x).sum()), total + int(touching.sum())
            assert (carrying & ~x).any()
    print("%s under GJK + EPA: device against the model %.1f; %d of %d touching body-substeps checked" % (name, worst, checked, total))
    assert total >= (30 if name.startswith("exact") else 50) and checked >= 0.5 * total


def test_without_set_sleeping_the_same_frames_leave_the_bound():
    """The control: the same start states in a world in which everybody is awake."""
    name = "general-h1200"
    frames = run(name, frames=2)
    worst = 0.0
    with xd.new_world() as w:
        for f, (start, _, res, x, c, links, s) in enumerate(frames):
            reach(w, dict(s, bodies=start), sleeping=False)
            w.step(s["h"], 1)
            got = w.download()[:len(start)]
            worst = max(worst, np.where(x, 0, sc.errors(s, got, res, start) / sc.bounds(res)).max())
    print("%s with nobody asleep: %.3g x the bound" % (name, worst))
    assert worst > 1.0
