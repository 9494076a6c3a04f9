"""Damping (stage 7) and the kinematic overwrite (stage 0), shared by test_xprec_damping_oracle.py (f64 evaluation vs the
longdouble model, CPU) and test_gpu_xprec_damping.py (HIP vs the model): the scenes, each a sequence of SINGLE-SUBSTEP frames
(dt = h, substeps = 1) that its builder re-makes frame by frame as xprec_bounce_cases.py does, the model
(xprec_pairs_model.substep with kinematics=, substeps_left=, damping= and joint_damping=), the bound and the exclusions.
Builders, normalisation, bounds and caps are those of xprec_bounce_cases.py and the files it rests on.

Scenes, 40 bodies or fewer each, 12 frames (`chain`: 8), at h = 1/1200 and 1/240 (`exact`: 2^-10 and 2^-8):
  (a) drag       xprec_bounce_cases.scene_bounce (clusters bouncing on the ground and on each other, restitution on); per body
                 c_l, c_a from {0, 0.5, 5, 50, 2000} 1/s, caps +inf; body 1 keeps the default row
  (b) caps       scene (a), and per body and frame each cap {inf, 0.25, 0.9, 1.1, 4} times that body's own speed after stage 6 in the
                 f64 evaluation of the frame without stage 7; a cap whose cap_margin would lie in (0, TAU] is redrawn (REDRAWN
                 counts them: none was)
  (c) dampers    `jointed`: xprec_bounce_cases.scene_jointed and one static box, a rod from it to cluster 0's C and a rod from
                 cluster 0's B to cluster 1's A (B then has three joints); `chain`: xprec_bounce_cases.scene_chain.  Joint j has a
                 linear damper (j % 4 == 0), an angular one (1), both (2) or none (3; joint 3 is LISTED with 0, 0), mu from
                 {10, 200, 5000} 1/s; the rows of (a) on the even bodies
  (d) exact      binary-exact states, no gravity, far from the ground: EXACT_* below names each case
  (e) platforms  kinematic bodies that push and carry, MUS, GROUND_MU and restitution on: POSE slabs that rise (one rider at rest,
                 e = 0.8), fall away and translate, a POSE turntable turning 1e-3 to 0.5 rad in the substep, a VELOCITY conveyor
                 and a VELOCITY spinner, each under riders; hovering kinematic boxes under one rider each: a center_of_mass of
                 (0.3, -0.2, 0.1), a target rotation of length 3.7, a target with dq.s < 0, a target equal to the pose; a
                 kinematic box crossing the ground and a static box in it; a kinematic box with a hinged box (ANGLE drive,
                 damper) and a third box on a damped ball joint.  Every kinematic body is stored with a velocity of (0.3, -0.2, 0.7)
                 and a spin of (0.1, 0.2, -0.3) that the overwrite must replace
  (f) all        scene (e) with (b)'s rows on the dynamic bodies, a drag row on the conveyor (a fixed body: no effect) and (e)'s
                 dampers

MEASURED: see below."""
import functools

import numpy as np

import xprec_bounce_cases as bc
import xprec_check as xk
import xprec_drives_cases as dc
import xprec_joints_cases as jc
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from constraint_solver_amd import capi
from xprec_cases import COND_MIN, FLIP_MIN, TAU
from xprec_pairs_cases import CUBE, GROUND_MU, HS, MUS, SLAB

# MEASURED, largest normalised error of a checked body-substep, f64 evaluation against the longdouble model, h = 1/1200 and 1/240
# (test_xprec_damping_oracle.py prints them; in brackets the body-substeps WITHOUT a one-point stage-6 entry):
#   drag 21.6 (3.7) and 31.0 (11.6)      caps 19.8 (3.4) and 17.3 (11.6)     jointed 12.3 (5.1) and 17.2 (7.8)
#   chain 14.2 (7.9) and 7.9 (18.1)      platforms 11.4 (1.8) and 25.0 (4.7)  all 10.3 (1.1) and 20.7 (4.7)
#   exact 0.7 at h = 2^-10 and 2^-8
# 8 x the maximum fits under xprec_bounce_cases.bounds() UNCHANGED: 8 x 31.0 = 248 < K_BOUNCE = 17 931 on a body with a one-point
# stage-6 entry, 8 x 18.1 = 145 < K_PLAIN = 946 on every other one; a test keeps both.  No new bound: stage 7 multiplies
# velocities by factors in (0, 1] and adds terms lambda n with n = d / len, len a relative SPEED of 1e-2 to 10 m/s here, never the
# millimetre penetration that makes stage 6's one-point normal ill-conditioned, and the overwrite is a quotient and one tan.
# The 40-digit mpmath model moves the frame that holds each scene's maximum by 0.0073 at most (7.7e-6 of K_PLAIN).
# Excluded: 2 of 5 056 body-substeps (platforms-h240, the rider of `holds` in frames 2 and 7: a one-ulp sensitivity of 11.0 and
# 12.0, above SENSITIVITY_MAX), 0 of the 2 636 that carry a damper entry or a fired cap (scene (a), which has neither by
# construction, counts its 444 body-substeps with a non-zero drag coefficient instead; scene (e) has 24 per h, the others 48 to
# 324).  No cap was redrawn (REDRAWN: 0 in the 48 frames of (b) and (f)).
# Seeds, the first ones tried, none changed after a figure was seen: 101 (scenes (a), (b), jointed: xprec_bounce_cases'), 3
# (chain), 201 (drag rows), 301 (cap factors), 211 and 221 (damper coefficients), 401 (platforms), 4100 (lone entries).
# Two things WERE changed after a first look, both before any comparison with the device: the two boxes in the ground of scene
# (e) had drawn mu = 0, which makes the friction margin of a body that cannot slide exactly 0 and excluded them (now 0.5); and
# the stage-7 reading "entries summed" had the name of stage 6's and ran both (renamed damper_entries_summed).
# Lone POSE entries (lone_chain), largest normalised POSE error of a checked body, f64 chain against the longdouble chain:
#   S = 1: 0.2345   S = 3: 0.3036   S = 20: 0.1440; K_LONE is 8 x that.  Excluded: entry HALF_TURN (dq.s == 0 exactly).
# The longdouble chain ends 2.2e-21 (position, relative) and 1.6e-19 (rotation) from the target at most.
SUBSTEPS = 12
MAX_BODIES = 40
EXACT_HS = (2.0 ** -10, 2.0 ** -8)
DRAGS = np.array([0.0, 0.5, 5.0, 50.0, 2000.0])
CAP_FACTORS = np.array([np.inf, 0.25, 0.9, 1.1, 4.0])
DAMPER_MUS = np.array([10.0, 200.0, 5000.0])
TURNS = (1e-3, 1e-2, 0.05, 0.1, 0.3, 0.5)
STORED_VELOCITY, STORED_SPIN = (0.3, -0.2, 0.7), (0.1, 0.2, -0.3)
REDRAWN = {}                       # (scene, frame) -> caps redrawn because their margin lay in (0, TAU]


def drag_rows(n, seed, keep_default=()):
    rng = np.random.default_rng(seed)
    rows = capi.body_damping(n, DRAGS[rng.integers(0, len(DRAGS), n)], DRAGS[rng.integers(0, len(DRAGS), n)])
    for b in keep_default:
        rows[b] = capi.body_damping(1)[0]
    return rows


def pattern_dampers(n_joints, seed):
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n_joints):
        mu_l, mu_a = DAMPER_MUS[rng.integers(0, 3)], DAMPER_MUS[rng.integers(0, 3)]
        kind = j % 4
        if kind == 3 and j != 3:
            continue
        out.append((j, 0.0 if kind in (1, 3) else mu_l, 0.0 if kind in (0, 3) else mu_a))
    j, mu_l, mu_a = (np.array(x) for x in zip(*out))
    return capi.joint_damping(j, mu_l, mu_a)


# ---- (a) drag, (b) caps -----------------------------------------------------------------------------------------------------
def scene_drag(h, frame, seed=101):
    s = bc.scene_bounce(h, frame, seed)
    return dict(s, rows=drag_rows(len(s["sid"]), 201, keep_default=(1,)))


def speeds_after_stage_6(s):
    """Per body (|v|, |w|) of the f64 evaluation of the scene's substep without stage 7."""
    state = xm.f64().to_f64(evaluate(s, num=xm.f64(), without=("damping", "joint_damping"))["state"])
    return np.linalg.norm(state[:, 22:25], axis=1), np.linalg.norm(state[:, 25:28], axis=1)


def with_caps(s, tag, bodies=None, seed=301):
    """The scene with caps drawn per body: a factor of CAP_FACTORS times the body's own speed after stage 6."""
    n = len(s["sid"])
    rng = np.random.default_rng(seed)
    factors = CAP_FACTORS[rng.integers(0, len(CAP_FACTORS), (n, 2))]
    speed = np.stack(speeds_after_stage_6(s), axis=1)
    rows = s["rows"].copy()
    chosen = np.arange(n) if bodies is None else np.asarray(bodies)
    redrawn = 0
    for attempt in range(8):
        cap = np.where(np.isfinite(factors) & (speed > 0), factors * np.where(speed > 0, speed, 1.0), np.inf)
        rows["max_linear_speed"][chosen], rows["max_angular_speed"][chosen] = cap[chosen, 0], cap[chosen, 1]
        margin = evaluate(dict(s, rows=rows), num=xm.f64())["cap_margin"]
        close = np.nonzero(xk.in_band(margin))[0]
        if not len(close):
            break
        redrawn += len(close)
        factors[close] = CAP_FACTORS[rng.integers(0, len(CAP_FACTORS), (len(close), 2))]
    REDRAWN[tag] = redrawn
    return dict(s, rows=rows)


def scene_caps(h, frame, seed=101):
    return with_caps(finish(scene_drag(h, frame, seed), h, False), ("caps", h, frame))


# ---- (c) dampers ------------------------------------------------------------------------------------------------------------
def scene_dampers_jointed(h, frame, seed=101):
    s = bc.scene_jointed(h, frame, seed)
    static = pc.new_body(CUBE, s["bodies"][2][31:34] + np.array([0.0, 0.0, 6.0]), static=True)
    bodies = np.concatenate([s["bodies"], static[None]])
    n = len(bodies)
    extra = jc.joints_of([jc.rod(bodies, n - 1, 2, (0.5, 0.5, 0.0), (0.3, 0.2, 0.1), 0.01),
                          jc.rod(bodies, 1, 3, (0.2, 0.3, 0.1), (0.1, 0.2, 0.3), 0.01)])
    joints = np.concatenate([s["joints"], extra])
    rows = drag_rows(n, 201)
    rows[1::2] = capi.body_damping(1)[0]
    return dict(s, bodies=bodies, sid=np.append(s["sid"], CUBE).astype(np.uint32), labels=np.append(s["labels"], "static"),
                e=np.append(s["e"], 0.0), mu=np.append(s["mu"], 0.5), joints=joints, rows=rows,
                dampers=pattern_dampers(len(joints), 211))


def scene_dampers_chain(h, frame, seed=3):
    s = bc.scene_chain(h, frame, seed)
    rows = drag_rows(len(s["sid"]), 201)
    rows[1::2] = capi.body_damping(1)[0]
    return dict(s, rows=rows, dampers=pattern_dampers(len(s["joints"]), 221))


# ---- (d) exact --------------------------------------------------------------------------------------------------------------
EXACT_CAP_TIE, EXACT_ALIKE, EXACT_FIXED, EXACT_K_ONE, EXACT_NO_DRAG = 0, (1, 2), (3, 4), (5, 6), 7
EXACT_JOINT_ALIKE, EXACT_JOINT_FIXED, EXACT_JOINT_K_ONE = 0, 1, 2


def scene_exact(h, frame):
    """0: v = (3, 4, 0) / 8, no drag, cap 5 / 8: m == cap, and the stated m > cap does not fire.  1, 2: a rod between the two
    bodies' centres of mass (center_of_mass 0, anchors 0: the arm is 0), both moving alike, 2 turning: no linear term, an angular
    term, one entry with count 1.  3, 4: both ends fixed, both coefficients set: no term, no NaN.  5, 6: mu_l = 1 / h exactly:
    k == 1.0.  7: c == 0 and caps that do not fire: every bit of the undamped evaluation."""
    z = 8.0 + frame * 2.0 ** -3
    kw = {"gravity": False}
    bodies = [pc.new_body(CUBE, (0.0, 0.0, z), velocity=(0.375, 0.5, 0.0), **kw),
              pc.new_body(CUBE, (8.0, 0.0, z), velocity=(0.25, 0.0, 0.0), **kw),
              pc.new_body(CUBE, (10.0, 0.0, z), velocity=(0.25, 0.0, 0.0), spin=(0.0, 0.0, 0.5), **kw),
              pc.new_body(CUBE, (16.0, 0.0, z), velocity=(0.25, 0.0, 0.0), spin=(0.5, 0.0, 0.0), static=True),
              pc.new_body(CUBE, (18.0, 0.0, z), velocity=(-0.25, 0.0, 0.0), static=True),
              pc.new_body(CUBE, (24.0, 0.0, z), velocity=(0.0, 0.25, 0.0), **kw),
              pc.new_body(CUBE, (26.0, 0.0, z), velocity=(0.0, -0.25, 0.0), spin=(0.0, 0.25, 0.0), **kw),
              pc.new_body(CUBE, (32.0, 0.0, z), velocity=(0.3, -0.1, 0.2), spin=(0.4, 0.1, -0.2), **kw)]
    bodies = np.array(bodies)
    bodies[1:3, 28:31] = 0.0
    zero = (0.0, 0.0, 0.0)
    joints = jc.joints_of([dict(body_a=1, body_b=2, anchor_a=zero, anchor_b=zero, distance=2.0),
                           dict(body_a=3, body_b=4, anchor_a=zero, anchor_b=zero, distance=2.0),
                           dict(body_a=5, body_b=6, anchor_a=(0.5, 0.5, 0.5), anchor_b=(0.5, 0.5, 0.5), distance=2.0)])
    rows = capi.body_damping(len(bodies))
    rows[EXACT_CAP_TIE]["max_linear_speed"] = 0.625
    rows[EXACT_NO_DRAG]["max_linear_speed"] = rows[EXACT_NO_DRAG]["max_angular_speed"] = 100.0
    dampers = capi.joint_damping([0, 1, 2], [16.0, 16.0, 1.0 / h], [16.0, 16.0, 0.0])
    n = len(bodies)
    return {"bodies": bodies, "sid": np.zeros(n, dtype=np.uint32), "labels": np.array(["tie", "alike", "alike", "fixed", "fixed",
            "k-one", "k-one", "no-drag"]), "e": np.zeros(n), "mu": None, "exact": (0, 1, 2), "joints": joints, "rows": rows,
            "dampers": dampers, "ground_e": 0.0}


# ---- (e) platforms ----------------------------------------------------------------------------------------------------------
def quat(q1, q2):
    return np.array(xm.qmul(np.asarray(q1, dtype=np.float64)[:, None], np.asarray(q2, dtype=np.float64)[:, None]))[:, 0]


def scene_platforms(h, frame, seed=401):
    rng = np.random.default_rng(seed * 1000 + frame)
    bodies, sid, labels, e, table = [], [], [], [], []

    def add(body, shape, label, restitution):
        bodies.append(body), sid.append(shape), labels.append(label), e.append(restitution)
        return len(bodies) - 1

    def scripted(body, shape, label, mode, linear, angular, moving=(0.0, 0.0, 0.0)):
        """A fixed body with a table entry; `moving`: the velocity its riders are placed against."""
        body[22:25] = moving
        k = add(body, shape, label, 0.3)
        table.append((k, mode, linear, angular))
        return k

    def rider(k, direction, label, at_rest=False):
        base = bodies[k]
        r = pc.new_body(CUBE, base[31:34], jc.tilt(rng, 0.1), spin=bc.spin(rng, 0.5))
        if at_rest:                                       # a gap of 0.2 to 0.8 of what the base rises in the substep
            bc.approach(rng, base, sid[k], r, CUBE, direction, h, (1.0, 1.0))
            r[22:28] = 0.0
        else:
            bc.approach(rng, base, sid[k], r, CUBE, direction, h, (0.5, 3.0))
        return add(r, CUBE, label, 0.8 if at_rest else bc.ES[1 + rng.integers(0, 3)])

    ident = np.array([1.0, 0.0, 0.0, 0.0])
    left, right = (-0.45, 0.05, 1.0), (0.45, -0.1, 1.0)
    # POSE slabs: rise, fall away, translate; the turntable
    for unit, (label, v) in enumerate((("rise", (0.0, 0.0, 1.0)), ("fall", (0.0, 0.0, -0.5)), ("translate", (1.5, 0.5, 0.0)))):
        slab = pc.new_body(SLAB, (12.0 * unit, 0.0, -3.5), static=True)
        k = scripted(slab, SLAB, label, capi.KINEMATIC_POSE, slab[31:34] + np.array(v) * h, ident, v)
        rider(k, left, label + "-rider", at_rest=label == "rise")
        rider(k, right, label + "-rider")
    slab = pc.new_body(SLAB, (36.0, 0.0, -3.5), static=True)
    k = scripted(slab, SLAB, "turntable", capi.KINEMATIC_POSE, slab[31:34], jc.yaw(TURNS[frame % len(TURNS)]))
    rider(k, left, "turntable-rider"), rider(k, right, "turntable-rider")
    # VELOCITY: a conveyor and a spinner
    slab = pc.new_body(SLAB, (48.0, 0.0, -3.5), static=True)
    k = scripted(slab, SLAB, "conveyor", capi.KINEMATIC_VELOCITY, (1.0, 0.5, 0.0), (0.0, 0.0, 0.0, 0.0), (1.0, 0.5, 0.0))
    rider(k, left, "conveyor-rider")
    slab = pc.new_body(SLAB, (60.0, 0.0, -3.5), static=True)
    k = scripted(slab, SLAB, "spinner", capi.KINEMATIC_VELOCITY, (0.0, 0.0, 0.0), (0.1, -0.05, 2.0, 7.0))
    rider(k, right, "spinner-rider")
    # hovering POSE boxes under one rider each
    for unit, label in enumerate(("com", "long", "far-side", "holds")):
        q = pc.random_rotation(rng)
        box = pc.new_body(CUBE, (12.0 * unit, 20.0, 6.0), q, static=True)
        v = np.array([0.5, -0.3, 0.2])
        p_t, q_t = box[31:34] + v * h, quat(jc.tilt(rng, 0.05), q)
        if label == "com":
            box[28:31] = (0.3, -0.2, 0.1)
        elif label == "long":
            q_t = 3.7 * q_t
        elif label == "far-side":
            q_t = -q_t
        elif label == "holds":
            p_t, q_t, v = box[31:34].copy(), q.copy(), np.zeros(3)
        k = scripted(box, CUBE, label, capi.KINEMATIC_POSE, p_t, q_t, v)
        rider(k, (0.05, 0.1, 1.0), label + "-rider")
    # a kinematic box that crosses the ground in the substep and a static box in it
    box = pc.new_body(CUBE, (0.0, 40.0, 0.4 * h), static=True)
    scripted(box, CUBE, "crossing", capi.KINEMATIC_POSE, box[31:34] - np.array([0.0, 0.0, 1.0]) * h, ident)
    add(pc.new_body(CUBE, (12.0, 40.0, -0.25), static=True), CUBE, "static", 0.3)
    # a kinematic box, a box hinged to it (ANGLE drive, damper) and a third on a damped ball joint
    q = pc.random_rotation(rng)
    box = pc.new_body(CUBE, (24.0, 40.0, 6.0), q, static=True)
    root = scripted(box, CUBE, "root", capi.KINEMATIC_POSE, box[31:34] + np.array([0.3, 0.2, -0.1]) * h, quat(jc.tilt(rng, 0.02), q))
    first = add(pc.new_body(CUBE, (25.3, 40.0, 6.0), jc.tilt(rng, 0.1), velocity=rng.uniform(-0.5, 0.5, 3), spin=bc.spin(rng)), CUBE, "hinged", 0.3)
    second = add(pc.new_body(CUBE, (26.6, 40.0, 6.0), jc.tilt(rng, 0.1), velocity=rng.uniform(-0.5, 0.5, 3), spin=bc.spin(rng)), CUBE, "hinged", 0.3)
    for k in [t[0] for t in table]:                       # what the overwrite must replace
        bodies[k][22:25], bodies[k][25:28] = STORED_VELOCITY, STORED_SPIN
    rows = [dc.hinge(bodies, root, first, (25.15, 40.5, 6.5), (0.1, 1.0, 0.2), rng.uniform(-0.005, 0.005, 3), rng.normal(size=3) * 0.02),
            jc.ball(bodies, first, second, (26.45, 40.5, 6.5), rng.uniform(-0.005, 0.005, 3))]
    drives = dc.drives_of([dict(joint=0, kind=capi.DRIVE_ANGLE, target=0.3, compliance=1e-3, **dc.refs(bodies, rows[0], 0.1))])
    n = len(bodies)
    fixed = np.random.default_rng(seed)
    kin = capi.kinematics([t[0] for t in table], [t[1] for t in table], [t[2] for t in table],
                          [np.asarray(t[3], dtype=np.float64) for t in table])
    mu = MUS[fixed.integers(0, len(MUS), n)]
    mu[[labels.index("crossing"), labels.index("static")]] = 0.5      # (mu = 0 on a body that cannot slide: a friction margin of 0)
    return {"bodies": np.array(bodies), "sid": np.array(sid, dtype=np.uint32), "labels": np.array(labels), "e": np.array(e),
            "mu": mu, "exact": (), "joints": jc.joints_of(rows), "drives": drives,
            "kinematics": kin, "dampers": capi.joint_damping([0, 1], [200.0, 10.0], [200.0, 5000.0])}


def scene_all(h, frame, seed=401):
    s = finish(scene_platforms(h, frame, seed), h, True)
    n = len(s["sid"])
    rows = drag_rows(n, 201)
    dynamic = np.nonzero(s["bodies"][:, 0] > 0)[0]
    conveyor = int(np.nonzero(s["labels"] == "conveyor")[0][0])
    for b in range(n):
        if b not in dynamic and b != conveyor:
            rows[b] = capi.body_damping(1)[0]
    rows[conveyor] = capi.body_damping(1, 5.0, 5.0)[0]
    return with_caps(dict(s, rows=rows), ("all", h, frame), bodies=dynamic)


# name -> (builder(h, frame), h, friction?)
def _scenes():
    out = {}
    for h in HS:
        tag = "h%d" % round(1.0 / h)
        out["drag-" + tag] = (scene_drag, h, False)
        out["caps-" + tag] = (scene_caps, h, False)
        out["jointed-" + tag] = (scene_dampers_jointed, h, False)
        out["chain-" + tag] = (scene_dampers_chain, h, False)
        out["platforms-" + tag] = (scene_platforms, h, True)
        out["all-" + tag] = (scene_all, h, True)
    for h in EXACT_HS:
        out["exact-h%d" % round(1.0 / h)] = (scene_exact, h, False)
    return out


SCENES = _scenes()


def finish(s, h, friction):
    """The builder's dict with every field the model and the device runs read."""
    s = dict(s)
    assert len(s["sid"]) <= MAX_BODIES
    s.setdefault("joints", bc.NO_JOINTS)
    s.setdefault("limits", jc.NO_LIMITS)
    s.setdefault("drives", dc.NO_DRIVES)
    s.setdefault("threshold", 0.0 if h in (HS[0], EXACT_HS[0]) else 0.5)
    s.setdefault("ground_e", bc.GROUND_E)
    s.setdefault("rows", None)
    s.setdefault("dampers", None)
    s.setdefault("kinematics", None)
    s.update(h=h, speed=0.0, mu=s["mu"] if friction else None, ground_mu=GROUND_MU if friction else np.inf, terrain=None)
    s["ext"] = np.maximum(pc.extents(s["sid"], s["bodies"]), jc.arms(s))
    return s


@functools.lru_cache(maxsize=None)
def build(name, frame):
    builder, h, friction = SCENES[name]
    return finish(builder(h, frame), h, friction)


def evaluate(s, state=None, num=None, mutation=None, tau=0.0, manifolds=None, without=(), substeps_left=1, substep_index=0):
    """The model's substep of a finished scene (from `state` if given).  without: "damping", "joint_damping", "kinematics"."""
    return pm.substep(s["bodies"] if state is None else state, pc.table()[1], s["sid"], s["h"], manifolds, s["mu"], s["ground_mu"],
                      s["speed"], num=num, mutation=mutation, tau=tau, joints=s["joints"], limits=s["limits"], drives=s["drives"],
                      restitution=s["e"], ground_restitution=s["ground_e"], bounce_threshold=s["threshold"],
                      kinematics=None if "kinematics" in without else s["kinematics"], substeps_left=substeps_left,
                      damping=None if "damping" in without else s["rows"],
                      joint_damping=None if "joint_damping" in without else s["dampers"], substep_index=substep_index)


def model(name, frame, **kw):
    return evaluate(build(name, frame), **kw)


def errors(name, frame, got, res):
    s = build(name, frame)
    return xk.scene_errors(s, got, res, s["bodies"])


def excluded(res, s):
    """xprec_bounce_cases.excluded, and the two stages' own: cap_margin in (0, TAU]; damper_cond in (0, COND_MIN) (a term's
    direction is d / len; exactly 0 is the stated skip); a kinematic body whose |dq.s| is below FLIP_MIN or whose half / r is
    within TAU of tan's pole, and with it every body that touches it or is jointed to it.  The clamp of k, drag and Wsum > 0
    exclude nothing."""
    x = bc.excluded(res, s["exact"])
    if "cap_margin" in res:
        x = x | xk.in_band(res["cap_margin"]) | ((res["damper_cond"] > 0) & (res["damper_cond"] < COND_MIN))
    if "kin_flip_margin" in res:
        bad = (res["kin_flip_margin"] < FLIP_MIN) | (res["kin_tan_margin"] < TAU)
        for i, j in xk.joint_links(s, res):
            if bad[i] or bad[j]:
                x[i] = x[j] = True
        x = x | bad
    return x


def bounds(res):
    return bc.bounds(res)


def is_fixed(s):
    return ~s["bodies"][:, 0:10].any(axis=1)


def carries(name, res, s):
    """The body-substeps the second cap counts: those with a stage-7 damper entry or a fired cap.  Scene (a) has neither by
    construction (no joints, caps +inf): there a body counts whose row has a non-zero drag coefficient."""
    if "n_damper_entries" not in res:
        return np.zeros(len(res["mask"]), dtype=bool)
    c = ((res["n_damper_entries"] > 0) & ~is_fixed(s)) | res["cap_fired_linear"] | res["cap_fired_angular"]
    if name.startswith("drag"):
        c = c | (s["rows"]["linear"] > 0) | (s["rows"]["angular"] > 0)
    return c


def frames_of(name):
    return jc.CHAIN_SUBSTEPS if name.startswith("chain") else SUBSTEPS


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """Returns dict(h=, frames=[(start, want, res, scene)]): `want` the f64 evaluation's state after the substep, res the
    longdouble model's result from `start` with its one-ulp sensitivity, scene = build(name, f)."""
    out = []
    chain = name.startswith("chain")
    for f in range(frames_of(name)):
        s = build(name, f)
        res, want = xk.model_frame(s, functools.partial(evaluate, s), s["bodies"], f, s["exact"], nudge_on_res_manifolds=chain)
        out.append((s["bodies"], want, res, s))
    return {"h": SCENES[name][1], "frames": out}


def check_states(name, got_states):
    """got_states[f]: the state after frame f of an implementation under test.  Asserts bounds() on every body-substep that is
    not excluded; returns (normalised errors, excluded, carries), each a list over frames of (n,) arrays."""
    frames = [(start, res, s) for start, _, res, s in trajectory(name)["frames"]]
    return xk.check_frames(name, frames, got_states, errors=xk.scene_errors, excluded=excluded, bound=bounds,
                           carries=lambda res, s: carries(name, res, s))

SEEN_BOTH_WAYS = {"a linear cap that fires", "a linear cap that does not fire", "an angular cap that fires",
                  "an angular cap that does not fire", "mu_l h below 1", "mu_l h at or above 1", "mu_a h below 1",
                  "mu_a h at or above 1", "a linear-only entry", "an angular-only entry", "a two-term entry",
                  "ends with unequal counts", "a damper with one end fixed", "a damped body with a stage-6 entry",
                  "a POSE entry with a contact", "a VELOCITY entry with a contact", "the negated dq"}


def seen(names):
    tags = set()
    for name in names:
        for _, _, res, s in trajectory(name)["frames"]:
            ok = ~excluded(res, s)
            tags |= res.get("damping_seen", set())
            if "n_damper_entries" in res and "bounce_pair_entries" in res:
                both = (res["n_damper_entries"] > 0) & ~is_fixed(s) & ((res["bounce_pair_entries"] + res["bounce_ground_entries"]) > 0)
                if (both & ok).any():
                    tags.add("a damped body with a stage-6 entry")
            if "kin_mode" in res:
                for i, j in res["manifolds"]:
                    for a, b in ((i, j), (j, i)):
                        if res["kin_mode"][a] >= 0 and ok[b] and res["manifolds"][(i, j)]["p_ref"]:
                            tags.add("a %s entry with a contact" % ("POSE", "VELOCITY")[res["kin_mode"][a]])
                if (res["kin_negated"] & ok).any():
                    tags.add("the negated dq")
    return tags


# ---- lone POSE entries, r > 1 -------------------------------------------------------------------------------------------------
N_LONE = 65
LONE_DT = 1.0 / 60.0
LONE_SUBSTEPS = (1, 3, 20)
HALF_TURN, UNNORMALISED, MINUS_Q, SPINNER = 0, 1, 2, 3
# 8 x the largest normalised pose error of the f64 evaluation against the longdouble chain, per S (filled in from the CPU run)
K_LONE = {1: 1.876, 3: 2.43, 20: 1.153}


@functools.lru_cache(maxsize=None)
def lone_scene():
    """65 fixed unit boxes 10 m apart, 5 m up, randomly turned, each with a POSE entry: a target up to 2 m away per axis and any
    rotation away.  Entry HALF_TURN turns by pi from the identity (dq.s == 0), UNNORMALISED has |q_t| = 3.7, MINUS_Q has
    q_t == -q, SPINNER turns 2.5 rad about z."""
    rng = np.random.default_rng(4100)
    n = N_LONE
    at = np.stack([10.0 * (np.arange(n) % 9), 10.0 * (np.arange(n) // 9), np.full(n, 5.0)], axis=1)
    bodies = np.array([pc.new_body(CUBE, at[i], static=True) for i in range(n)])
    linear, angular = np.zeros((n, 3)), np.zeros((n, 4))
    for i in range(n):
        q, q_t = pc.random_rotation(rng), pc.random_rotation(rng)
        if i == HALF_TURN:
            q, q_t = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0])
        elif i == UNNORMALISED:
            q_t = 3.7 * q_t
        elif i == MINUS_Q:
            q_t = -q
        elif i == SPINNER:
            q, q_t = np.array([1.0, 0.0, 0.0, 0.0]), np.array([np.cos(1.25), 0.0, 0.0, np.sin(1.25)])
        bodies[i, 34:38] = q
        linear[i], angular[i] = at[i] + rng.uniform(-2.0, 2.0, 3), q_t
    return bodies, np.zeros(n, dtype=np.uint32), capi.kinematics(np.arange(n), capi.KINEMATIC_POSE, linear, angular)


def lone_chain(substeps, num=None, mutation=None, kinematics=None, bodies=None):
    """The model chained `substeps` times with substeps_left = S - k on the lone entries, the state carried in the model's scalars.
    Returns (the state after every substep [(n, 38) model scalars], excluded (n,) bool: a flip or tan margin of some substep too
    small).  What a frame shows from outside is the last state only; the earlier ones are the model's to compare."""
    start, sid, kin = lone_scene()
    kin = kin if kinematics is None else kinematics
    state = start if bodies is None else bodies
    h = LONE_DT / substeps
    bad = np.zeros(len(state), dtype=bool)
    states = []
    for k in range(substeps):
        res = pm.substep(state, pc.table()[1], sid[:len(state)], h, {}, num=num, kinematics=kin, substeps_left=substeps - k, mutation=mutation,
                         substep_index=k)
        bad |= (res["kin_flip_margin"] < FLIP_MIN) | (res["kin_tan_margin"] < TAU) | (res["flip_margin"] < FLIP_MIN)
        state = res["state"]
        states.append(state)
    return states, bad


def lone_pose_errors(got, want_state):
    """Normalised pose error per body of `got` (n, 38) f64 against the chain's state: positions by eps (|x| + extent), rotation
    components by eps (|x| + extent) / extent, as everywhere else."""
    start, sid, _ = lone_scene()
    num = xm.native()
    ext = pc.extents(sid, start)
    d = np.abs(num.to_f64(num.conv(got) - want_state))
    scale = np.maximum(np.linalg.norm(start[:, 31:34], axis=1), np.linalg.norm(got[:, 31:34], axis=1)) + ext
    return np.maximum(d[:, 31:34].max(axis=1) / (pc.EPS * scale), d[:, 34:38].max(axis=1) / (pc.EPS * scale / ext))
