"""Damping (stage 7) and the kinematic overwrite (stage 0): the f64 evaluation of the model against the extended-precision model
(xprec_pairs_model.substep with kinematics=, substeps_left=, damping= and joint_damping=), frame by frame; the existing f64
models (tests/damping_model.py, tests/kinematic_model.py) on their own scenes within the same bound; the 40-digit model on the
frames that hold the maxima; a mutation table; the caps and "seen" conditions of the scene set; the lone POSE entries chained
over S substeps; and mechanics of the model itself.  Scenes, bound, exclusions and the measured figures: xprec_damping_cases.py."""
import numpy as np
import pytest

import damping_common as dmc
import damping_model as dm
import kinematic_common as kc
import kinematic_model as km
import restitution_model as rm
import xprec_bounce_cases as bc
import xprec_check as xk
import xprec_damping_cases as dcs
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from constraint_solver_amd import capi
from golden_util import bits_equal

SCENE_NAMES = list(dcs.SCENES)


def f64_states(name):
    return [fr[1] for fr in dcs.trajectory(name)["frames"]]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_f64_reading_against_the_model_frame_by_frame(name):
    """Every checked body-substep of the f64 evaluation of the model is within bounds() of the longdouble model; the exclusion caps
    hold over all body-substeps and over those that carry a stage-7 damper entry or a fired cap; the exact scene does what the
    header says, case by case."""
    t = dcs.trajectory(name)
    errs, excl, entry = dcs.check_states(name, f64_states(name))
    x, c = np.concatenate(excl), np.concatenate(entry)
    print("%s: f64 evaluation %.1f; excluded %d of %d body-substeps, %d of %d that carry a damper entry or a fired cap" % (
        name, xk.worst(errs, excl), x.sum(), x.size, (x & c).sum(), c.sum()))
    xk.assert_caps(name, excl, entry)
    for f, (start, want, res, s) in enumerate(t["frames"]):
        assert len(start) <= dcs.MAX_BODIES and not np.isnan(want).any()
        if name.startswith("drag"):
            assert not s["rows"][1]["linear"] and not s["rows"][1]["angular"] and (s["rows"]["linear"] * s["h"] > 1).any()
            assert ((s["rows"]["linear"] > 0) & (s["rows"]["linear"] * s["h"] < 1)).any()
        if name.startswith("exact"):
            plain = xm.f64().to_f64(dcs.model(name, f, num=xm.f64(), without=("damping", "joint_damping"))["state"])
            tie = dcs.EXACT_CAP_TIE                                      # m == cap: the stated m > cap does not fire
            assert res["cap_margin"][tie] == 0.0 and not res["cap_fired_linear"][tie] and bits_equal(want[tie], plain[tie])
            a, b = dcs.EXACT_ALIKE                                       # anchors move alike, ends turn differently
            terms = {(j, kind): (k, length) for j, kind, k, length in res["damper_terms"]}
            assert (dcs.EXACT_JOINT_ALIKE, "linear") not in terms and (dcs.EXACT_JOINT_ALIKE, "angular") in terms
            assert res["n_damper_entries"][[a, b]].tolist() == [1, 1] and res["n_damper_terms"][[a, b]].tolist() == [1, 1]
            assert bits_equal(want[[a, b], 22:25], plain[[a, b], 22:25]) and not bits_equal(want[[a, b], 25:28], plain[[a, b], 25:28])
            a, b = dcs.EXACT_FIXED                                       # both ends fixed: no term, no NaN, nothing moves them
            assert not [k for k in terms if k[0] == dcs.EXACT_JOINT_FIXED]
            assert np.isfinite(want[[a, b]]).all() and bits_equal(want[[a, b]], plain[[a, b]])
            assert terms[(dcs.EXACT_JOINT_K_ONE, "linear")][0] == 1.0    # mu = 1 / h exactly: k == 1.0
            assert bits_equal(want[dcs.EXACT_NO_DRAG], plain[dcs.EXACT_NO_DRAG])      # c == 0: every bit
        if name.startswith(("platforms", "all")):
            labels = list(s["labels"])
            assert res["kin_zero"][labels.index("holds")] and res["kin_negated"][labels.index("far-side")]
            for label in ("crossing", "static"):
                k = labels.index(label)
                assert res["mask"][k] != 0 and np.isfinite(want[k]).all()     # in the ground: a contact, no effect, no NaN
            assert bits_equal(want[labels.index("static"), 31:38], start[labels.index("static"), 31:38])
            assert want[labels.index("crossing"), 33] < 0.0 < start[labels.index("crossing"), 33]
            rest = labels.index("rise-rider")                            # at rest on the rising slab: vn0 is the scripted velocity
            assert not start[rest, 22:28].any() and res["bounce_pair_entries"][rest] >= 1
    if name.startswith(("jointed", "chain")):
        s = t["frames"][0][3]
        joints, damped = s["joints"], {int(d["joint"]): (d["linear"], d["angular"]) for d in s["dampers"]}
        fixed = dcs.is_fixed(s)
        assert damped[3] == (0.0, 0.0)                                   # a joint listed with (0, 0)
        if name.startswith("jointed"):
            assert any(joints[j]["body_a"] > joints[j]["body_b"] and max(damped[j]) > 0 for j in damped)
            assert any(fixed[joints[j]["body_a"]] != fixed[joints[j]["body_b"]] and max(damped[j]) > 0 for j in damped)
            counts = t["frames"][0][2]["n_damper_entries"][~fixed]
            assert {1, 2, 3} <= set(counts.tolist())                     # bodies with one, two and three damped joints
        assert len(damped) < len(joints)                                 # undamped joints beside damped ones


def test_the_measured_maxima_fit_eight_times_under_the_existing_bounds():
    """8x the largest error of a checked body-substep fits under xprec_bounce_cases.bounds() unchanged: under K_BOUNCE on a body
    with a one-point stage-6 entry, under K_PLAIN on every other one.  No new bound is introduced."""
    with_one, others = 0.0, 0.0
    for name in SCENE_NAMES:
        a = b = 0.0
        for f, (start, want, res, s) in enumerate(dcs.trajectory(name)["frames"]):
            e = np.where(dcs.excluded(res, s), 0, dcs.errors(name, f, want, res))
            a, b = max(a, e[bc.one_point(res)].max(initial=0.0)), max(b, e[~bc.one_point(res)].max(initial=0.0))
        print("%s: %.1f with a one-point entry, %.1f without" % (name, a, b))
        with_one, others = max(with_one, a), max(others, b)
    print("largest normalised errors: %.1f (8x = %.0f, K_BOUNCE = %g), %.1f without a one-point entry (8x = %.0f, K_PLAIN = %g)" % (
        with_one, 8 * with_one, bc.K_BOUNCE, others, 8 * others, bc.K_PLAIN))
    assert 8 * with_one <= bc.K_BOUNCE and 8 * others <= bc.K_PLAIN
    assert sum(dcs.REDRAWN.values()) == 0 and len(dcs.REDRAWN) == 4 * dcs.SUBSTEPS     # no cap had to be redrawn


def test_the_scene_set_sees_everything():
    tags = dcs.seen(SCENE_NAMES)
    assert dcs.SEEN_BOTH_WAYS <= tags, dcs.SEEN_BOTH_WAYS - tags


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_longdouble_model_equals_mpmath_model(name):
    """The frame that holds the scene's largest error, on the longdouble model's manifolds, in longdouble and in 40-digit mpmath:
    the states agree 2^11 times inside the bound and within a tenth of that maximum, and stage 7 fires the same caps and makes the
    same entries: longdouble's rounding does not set the figure."""
    fast, ref = xm.native(), xm.mp(40)
    t = dcs.trajectory(name)
    errs, excl, _ = dcs.check_states(name, f64_states(name))
    per_frame = [float(np.where(x, 0, e).max()) for e, x in zip(errs, excl)]
    f = int(np.argmax(per_frame))
    start, _, res, s = t["frames"][f]
    given = {key: m for key, m in res["manifolds"].items() if m["p_ref"]}
    exact = {key: {"separated": False, "feature": m["feature"], "p_ref": [xm.lifted(ref, p) for p in m["p_ref"]],
                   "p_inc": [xm.lifted(ref, p) for p in m["p_inc"]], **({"normal": xm.lifted(ref, m["normal"])} if "normal" in m else {})}
             for key, m in given.items()}
    a = dcs.model(name, f, num=fast, manifolds=given)
    b = dcs.model(name, f, num=ref, manifolds=exact)
    for key in ("mask", "bounce_pair_entries", "bounce_ground_entries", "n_damper_entries", "n_damper_terms", "cap_fired_linear",
                "cap_fired_angular", "kin_zero", "kin_negated"):
        if key in a:
            assert np.array_equal(a[key], b[key]), key
    d = np.abs(ref.to_f64(xm.lifted(ref, a["state"]) - b["state"]))
    scale = pc.scales(start, fast.to_f64(a["state"]), s["ext"], xk.joint_links(s, res))
    turn = scale / s["ext"]
    h = s["h"]
    e = np.max(np.stack([d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * turn),
                         d[:, 22:25].max(axis=1) * h / (pc.EPS * scale), d[:, 25:28].max(axis=1) * h / (pc.EPS * turn)]), axis=0)
    print("%s frame %d: longdouble against mpmath %.4f = %.2g of K_PLAIN; the scene's maximum %.1f" % (
        name, f, e.max(), e.max() / bc.K_PLAIN, per_frame[f]))
    assert e.max() <= bc.K_PLAIN / 2 ** 11 and e.max() <= 0.1 * per_frame[f]


# The scene on which each wrong reading of the MODEL leaves the bound, and the measured factor (worst error / the body's bound).
CAUGHT_BY = {"drag_explicit": ("drag-h240", 4.4e11), "caps_before_drag": ("caps-h240", 4.7e9),
             "drag_before_dampers": ("jointed-h240", 2.5e10), "stage7_before_stage6": ("drag-h240", 2.2e10),
             "angular_on_linear_result": ("jointed-h240", 1.4e10), "neighbour_stage7_velocities": ("jointed-h240", 4.6e9),
             "count_is_terms": ("jointed-h240", 2.1e10), "damper_entries_summed": ("jointed-h240", 2.2e10),
             "k_unclamped": ("jointed-h240", 8.3e11), "damper_arm_without_com": ("jointed-h240", 1.5e10),
             "wang_unrotated": ("jointed-h240", 2.6e9), "anchors_at_integrated": ("chain-h240", 3.3e11),
             "fixed_body_damped": ("all-h240", 1.3e7), "cap_per_component": ("caps-h240", 4.6e9),
             "second_end_same_sign": ("jointed-h240", 4.5e10),
             "dq_conjugate_first": ("platforms-h240", 7.4e10), "full_angle": ("platforms-h240", 6.5e10),
             "overwrite_after_integrate": ("platforms-h240", 6.9e10), "p_frame_origin": ("platforms-h240", 7.4e11),
             "v0_before_overwrite": ("platforms-h240", 9.3e9)}
# Invisible on every single-substep scene, and why (each was tried on platforms-h1200, platforms-h240 and all-h240 first: 0.005 of
# the bound at most): `r_counted_up` and `velocity_once_per_frame` differ from the header only at k >= 1, and a single-substep
# frame has k = 0, r = 1; `dq_not_negated` is the same NUMBER at r = 1: without the negation half is pi - half' and vec(dq) has the
# other sign, and tan(pi - x) = -tan(x).  The negation matters only for r > 1, where half / r is another angle (the long way
# round).  All three are caught by the chained lone entries at S = 3 (LONE_CAUGHT_BY below), which the CPU can stop between
# substeps.  Invisible where they cannot act: caps_before_drag and cap_per_component without finite caps, every damper reading
# on scenes (a) and (b), fixed_body_damped without a fixed body that moves and has a row (scene (f)'s conveyor), wang_unrotated
# on scene (f) (its two damped joints hang on unit boxes whose inverse inertia is a multiple of the identity).


@pytest.mark.parametrize("mutation", list(CAUGHT_BY))
def test_the_bound_sees_each_misreading(mutation):
    """Each wrong variant of the model pushes the f64 evaluation beyond the bound on the named scene, on a body-substep that the
    true model checks."""
    name, factor = CAUGHT_BY[mutation]
    t = dcs.trajectory(name)
    worst = 0.0
    for f, (start, want, res, s) in enumerate(t["frames"]):
        wrong = dcs.model(name, f, mutation=mutation, manifolds=res["manifolds"])
        worst = max(worst, np.where(dcs.excluded(res, s), 0.0, dcs.errors(name, f, want, wrong) / dcs.bounds(res)).max())
    print("%s on %s: %.3g x the bound (recorded: %.2g)" % (mutation, name, worst, factor))
    assert worst > 1.0


def test_every_listed_misreading_has_a_row():
    assert set(CAUGHT_BY) | set(LONE_CAUGHT_BY) == set(pm.DAMPING_MUTATIONS + pm.KINEMATIC_MUTATIONS)


@pytest.mark.parametrize("name,without", [("drag-h1200", "damping"), ("caps-h1200", "damping"), ("jointed-h1200", "joint_damping"),
                                          ("chain-h1200", "joint_damping"), ("platforms-h1200", "kinematics")])
def test_the_bound_sees_each_setting(name, without):
    """The model without damping= leaves the bound of the full model on (a) and (b), without joint_damping= on (c), without
    kinematics= on (e): the device controls of test_gpu_xprec_damping.py, on the CPU reading."""
    t = dcs.trajectory(name)
    worst = 0.0
    for f in range(2):
        _, _, res, s = t["frames"][f]
        less = dcs.model(name, f, num=xm.f64(), without=(without,))
        worst = max(worst, np.where(dcs.excluded(res, s), 0, dcs.errors(name, f, xm.f64().to_f64(less["state"]), res) / dcs.bounds(res)).max())
    print("%s without %s: %.3g x the bound" % (name, without, worst))
    assert worst > 1.0


# ---- the lone POSE entries, r > 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", dcs.LONE_SUBSTEPS)
def test_lone_pose_entries_arrive_and_the_f64_chain_stays_within_the_recorded_bound(substeps):
    """The 65 lone POSE entries, the model chained S times with substeps_left = S - k: the f64 evaluation's end pose against the
    longdouble chain's (K_LONE[S] is 8x the figure printed here), and the longdouble chain ends within 1e-17 relative of the
    target: the definition is an exact inverse of integrate's rotation update."""
    num = xm.native()
    _, _, kin = dcs.lone_scene()
    ref, bad = dcs.lone_chain(substeps)
    got, _ = dcs.lone_chain(substeps, num=xm.f64())
    e = np.where(bad, 0.0, dcs.lone_pose_errors(xm.f64().to_f64(got[-1]), ref[-1]))
    print("S = %d: f64 chain against the longdouble chain %.4f (8x = %.3f, K_LONE = %g); excluded %s" % (
        substeps, e.max(), 8 * e.max(), dcs.K_LONE[substeps], np.nonzero(bad)[0]))
    assert np.nonzero(bad)[0].tolist() == [dcs.HALF_TURN]                 # dq.s == 0: the one entry whose way round is a tie
    assert 8 * e.max() <= dcs.K_LONE[substeps] <= 8.01 * e.max()
    p, q = ref[-1][:, 31:34], ref[-1][:, 34:38]
    q_t = num.conv(kin["angular"])
    q_t = q_t / np.sqrt((q_t * q_t).sum(axis=1))[:, None]
    sign = num.conv(np.sign(num.to_f64((q * q_t).sum(axis=1))))
    off_p = np.abs(num.to_f64(p - num.conv(kin["linear"]))).max(axis=1) / np.abs(kin["linear"]).max(axis=1)
    off_q = np.abs(num.to_f64(q - q_t * sign[:, None])).max(axis=1)
    print("S = %d: the longdouble chain ends %.2g (position, relative) and %.2g (rotation) from the target" % (
        substeps, off_p[~bad].max(), off_q[~bad].max()))
    assert off_p[~bad].max() <= 1e-17 and off_q[~bad].max() <= 1e-17


def lone_velocity_table():
    """VELOCITY entries on the first four lone boxes: they turn 0.02 to 0.3 rad per substep at S = 3."""
    spin = np.array([[0.0, 0.0, 4.0], [10.0, -20.0, 5.0], [0.0, 50.0, 0.0], [3.0, 1.0, -2.0]])
    return capi.kinematics(np.arange(4), capi.KINEMATIC_VELOCITY, [[0.5, 0.0, 0.1]] * 4, np.concatenate([spin, np.zeros((4, 1))], axis=1))


# misreading -> (what is chained at S = 3, the measured factor against K_LONE[3])
LONE_CAUGHT_BY = {"r_counted_up": ("pose", 5.6e14), "dq_not_negated": ("pose", 1.1e15), "velocity_once_per_frame": ("velocity", 1.5e12)}


@pytest.mark.parametrize("mutation", list(LONE_CAUGHT_BY))
def test_the_chained_lone_entries_see_the_readings_that_need_a_second_substep(mutation):
    """At S = 3, every substep's state of the f64 chain against the mutated longdouble chain, in the units of K_LONE[3]."""
    what, factor = LONE_CAUGHT_BY[mutation]
    kw = {} if what == "pose" else {"kinematics": lone_velocity_table()}
    got, _ = dcs.lone_chain(3, num=xm.f64(), **kw)
    ref, bad = dcs.lone_chain(3, **kw)
    wrong, _ = dcs.lone_chain(3, mutation=mutation, **kw)
    true = max(np.where(bad, 0.0, dcs.lone_pose_errors(xm.f64().to_f64(g), r)).max() for g, r in zip(got, ref))
    worst = max(np.where(bad, 0.0, dcs.lone_pose_errors(xm.f64().to_f64(g), w)).max() for g, w in zip(got, wrong))
    print("%s on the lone %s entries, S = 3: %.3g x K_LONE (recorded: %.2g); the true chain %.3g" % (
        mutation, what, worst / dcs.K_LONE[3], factor, true / dcs.K_LONE[3]))
    assert true <= dcs.K_LONE[3] < worst


# ---- mechanics of the model itself --------------------------------------------------------------------------------------------
def free_pair(spin=True):
    a = pc.new_body(pc.CUBE, (0.0, 0.0, 8.0), pc.random_rotation(np.random.default_rng(1)), velocity=(1.0, 0.2, 0.0),
                    spin=(0.3, -0.2, 0.5) if spin else (0, 0, 0), gravity=False)
    b = pc.new_body(pc.CUBE, (3.0, 0.1, 8.2), pc.random_rotation(np.random.default_rng(2)), velocity=(-0.5, 0.4, 0.3),
                    spin=(-0.4, 0.1, 0.2) if spin else (0, 0, 0), gravity=False)
    return np.array([a, b])


@pytest.mark.parametrize("mu", [10.0, 200.0, 5000.0])
def test_a_linear_damper_keeps_the_momentum_and_removes_k_of_the_relative_anchor_speed(mu):
    """damp() alone on a free pair with one joint: +lambda n and -lambda n, so the linear momentum is conserved to 1e-15, and with
    one entry per end the relative anchor speed along the term's direction after the pass is (1 - k) times the one before."""
    num = xm.native()
    bodies = free_pair()
    s = xm._unpack(bodies, num)
    h = num.const(1.0 / 240.0)
    joint = dict(body_a=0, body_b=1, anchor_a=(0.9, 0.4, 0.2), anchor_b=(0.1, 0.3, 0.8))
    pose, velocities = (s["position"], s["rotation"]), (s["velocity"], s["angular_velocity"])
    v, w, info = pm.damp(num, s, pose, velocities, [joint], None, capi.joint_damping([0], mu, 0.0), h)
    assert info["n_damper_entries"].tolist() == [1, 1]
    m = 1.0 / bodies[:, 0]
    before = (bodies[:, 22:25] * m[:, None]).sum(axis=0)
    after = (num.to_f64(v).T * m[:, None]).sum(axis=0)
    assert np.abs(after - before).max() <= 1e-15

    def relative(v, w):
        out = []
        for body, anchor in ((0, joint["anchor_a"]), (1, joint["anchor_b"])):
            x, q, com = s["position"][:, body], s["rotation"][:, body], s["center_of_mass"][:, body]
            p = xm.frame_apply(x + com + xm.qrot(q, -com), q, num.conv(np.array(anchor)))
            out.append(v[:, body] + xm.cross(w[:, body], p - (x + com)))
        return out[1] - out[0]

    k = min(mu / 240.0, 1.0)
    d0, d1 = relative(*velocities), relative(v, w)
    length = num.sqrt(xm.dot(d0, d0))                                    # along n = d0 / len: n . K n = Wsum is what lambda divides by
    assert abs(float(xm.dot(d1, d0) / length - length * num.const(1.0 - k))) <= 1e-15


def test_a_fired_cap_leaves_the_speed_at_the_cap():
    """After a fired cap length(v) <= cap (1 + 4 eps), in the f64 evaluation, for 200 random velocities and caps."""
    num = xm.f64()
    rng = np.random.default_rng(5)
    bodies = np.array([pc.new_body(pc.CUBE, (0.0, 0.0, 8.0), gravity=False)] * 200)
    bodies[:, 22:28] = rng.normal(size=(200, 6)) * 10.0 ** rng.uniform(-3, 3, (200, 1))
    caps = np.linalg.norm(bodies[:, 22:25], axis=1) * rng.uniform(0.01, 0.99, 200)
    caps_w = np.linalg.norm(bodies[:, 25:28], axis=1) * rng.uniform(0.01, 0.99, 200)
    s = xm._unpack(bodies, num)
    v, w, info = pm.damp(num, s, (s["position"], s["rotation"]), (s["velocity"], s["angular_velocity"]), [],
                         capi.body_damping(200, 0.0, 0.0, caps, caps_w), None, np.float64(1.0 / 240.0))
    assert info["cap_fired_linear"].all() and info["cap_fired_angular"].all()
    eps = 2.0 ** -52
    assert (np.linalg.norm(v.astype(np.longdouble), axis=0) <= caps * (1 + 4 * eps)).all()
    assert (np.linalg.norm(w.astype(np.longdouble), axis=0) <= caps_w * (1 + 4 * eps)).all()


# ---- the existing f64 models, held to this one --------------------------------------------------------------------------------
def against(step, state, shapes, sid, h, substeps, **settings):
    """`step(state) -> state` of an existing f64 model, `substeps` single substeps, each against this model from the same state.
    Returns (largest error / bound of a checked body-substep, fired caps, pair-contact points, excluded, total, the last result)."""
    r = np.array([np.linalg.norm(shapes[int(k)]["verts"], axis=1).max() for k in sid])
    worst, fired, entries, left_out, total = 0.0, 0, 0, 0, 0
    scene = {"exact": (), "joints": settings.get("joints", ())}
    for k in range(substeps):
        start = np.array(state, copy=True)
        ext = r + 2 * np.linalg.norm(start[:, 28:31], axis=1)
        state = step(start, k)
        res = pm.substep(start, shapes, sid, h, None, tau=pc.TAU, **{key: value(k) if callable(value) else value for key, value in settings.items()})
        e = pc.normalized_errors(state, res["state"], start, ext, h, xk.joint_links(scene, res))
        x = dcs.excluded(res, scene)
        worst = max(worst, float(np.where(x, 0, e / dcs.bounds(res)).max()))
        if "cap_fired_linear" in res:
            fired += int(res["cap_fired_linear"].sum() + res["cap_fired_angular"].sum())
        entries += int(res["n_points"].sum())
        left_out, total = left_out + int(x.sum()), total + x.size
    return worst, fired, entries, left_out, total, res


@pytest.mark.parametrize("name", ["pile", "pile_bouncing"])
def test_the_damping_model_lies_within_the_bound(name):
    """tests/damping_model.py on the two pile scenes the device is held to it on bit for bit (test_gpu_damping.py): after twelve
    substeps of its own, three substeps each against this model from the same state."""
    bodies, sid, joints, rows, dampers, e = dmc.scene(name)
    shapes = [pm.shape(p) for p in dmc.polys()]
    h = dmc.H
    if e is None:
        state = dm.oracle_substeps(bodies, sid, dmc.polys(), joints, 12 * h, 12, dmc.PAD, rows)
        step = lambda b, k: dm.oracle_substeps(b, sid, dmc.polys(), joints, h, 1, dmc.PAD, rows)      # noqa: E731
        settings = {}
    else:
        model = rm.Model(bodies, sid, dmc.polys(), e=[e] * len(bodies), ground_e=e)
        state = dm.restitution_substeps(model, 12 * h, 12, rows).copy()
        step = lambda b, k: dm.restitution_substeps(model, h, 1, rows).copy()                         # noqa: E731
        settings = {"restitution": np.full(len(bodies), e), "ground_restitution": e}
    worst, fired, _, left_out, total, _ = against(step, state, shapes, sid, h, 3, damping=rows, **settings)
    print("damping_model on %s against the model: %.3g of the bound, %d fired caps, %d of %d body-substeps excluded" % (
        name, worst, fired, left_out, total))
    assert worst <= 1.0 and fired >= 3 and left_out <= 0.10 * total


def test_the_kinematic_model_lies_within_the_bound():
    """tests/kinematic_model.py on the carried-box scene of test_gpu_kinematic.py (a box on a slab that a POSE entry translates,
    20 substeps a frame): after two substeps of its own, substeps 2, 3 and 4 of the frame (r = 18, 17, 16) each against this model
    from the same state.  (Not after twelve, as the pile scenes: the slab starts at 3 m/s, the box is kicked off it and from
    substep 6 of the first frame to the end of the third it touches nothing, so there the comparison would see no contact.)"""
    bodies, sid = kc.carry_scene()
    tbl = kc.carry_tables()[0]
    shapes = [pm.shape(p) for p in kc.polys()]
    S = kc.CARRY_SUBSTEPS
    h = kc.DT / S
    state = np.array(bodies, copy=True)
    own = 2
    for k in range(own):
        state, _ = km.overwrite(state, tbl, h, S - k)
        state = km.oracle_substeps(state, sid, kc.polys(), kc.NO_JOINTS, h, 1, kc.PAD)

    def step(b, k):
        b, _ = km.overwrite(b, tbl, h, S - own - k)
        return km.oracle_substeps(b, sid, kc.polys(), kc.NO_JOINTS, h, 1, kc.PAD)

    worst, _, points, left_out, total, res = against(step, state, shapes, sid, h, 3, kinematics=kc.to_capi(tbl),
                                                     substeps_left=lambda k: S - own - k)
    print("kinematic_model against the model: %.3g of the bound, %d contact points, %d of %d body-substeps excluded" % (
        worst, points, left_out, total))
    assert worst <= 1.0 and left_out == 0 and res["kin_mode"][0] == 0 and points >= 6                  # carried: contacts on the slab
