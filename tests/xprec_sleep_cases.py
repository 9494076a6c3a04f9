"""Awake bodies in contact with sleepers, shared by test_xprec_sleep_oracle.py (f64 evaluation vs the longdouble model, CPU) and
test_gpu_xprec_sleep.py (HIP vs the model): the scenes, each a sequence of SINGLE-SUBSTEP frames (dt = h, substeps = 1) that its
builder re-makes frame by frame as xprec_damping_cases.py does, the model (xprec_pairs_model.substep with asleep=), the chained
model for frames of S substeps, the bound and the exclusions.  Builders, normalisation, bounds and caps are those of
xprec_damping_cases.py and the files it rests on.

A scene names its sleepers (`asleep`) and its probes: the awake bodies that are moved into place before the frame under test.
On the CPU a sleeper is the builder's body at rest; on the device it is what the world's own sleep pass left (see
test_gpu_xprec_sleep.py), and the model is seeded from that download.

Scenes, 40 bodies or fewer each, FRAMES frames, at h = 1/1200 and 1/240 (`exact`: 2^-10):
  (a) general    eight sleepers -- boxes, hulls of 16 and 18 vertices, an icosahedron, a tetrahedron; floating with and without
                 gravity, and two on the ground -- with unequal masses; sleeper 0 has a center_of_mass of (0.3, -0.2, 0.1), three
                 times the mass and a non-unit box inertia; one or two probes of every shape class approach each
  (b) shared     a probe that reaches the ground, a sleeper and an awake body in the same substep, six times over
  (c) stack      three static slabs, on each a sleeping 3-stack of unit boxes (one group, a fixed anchor below it), a probe on
                 top and one against the side of the middle box
  (d) materials  scene (a) with mu per body from MUS, GROUND_MU, the depenetration limit 0 (`materials0`) and 3 m/s (`materials3`)
  (e) bouncing   scenes (a) and (c) with restitution per body from {0, 0.4, 0.8}, the sleepers included, and GROUND_E
  (f) damped     scene (a) with drag rows and finite caps on every body, the sleepers included
  (g) exact      binary-exact poses, no gravity, h = 2^-10: EXACT_* below names each case

MEASURED: see below."""
import functools

import numpy as np

import xprec_bounce_cases as bc
import xprec_check as xk
import xprec_damping_cases as dcs
import xprec_joints_cases as jc
import xprec_model as xm
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from xprec_cases import TAU
from xprec_pairs_cases import CUBE, G, HS, HULL16, HULL18, ICOSA, MUS, SLAB, TETRA

# MEASURED, largest normalised error of a checked body-substep, f64 evaluation against the longdouble model, h = 1/1200 and 1/240
# (test_xprec_sleep_oracle.py prints them): see DESIGN 1g, which holds the table; 8 x the maximum fits under
# xprec_bounce_cases.bounds() unchanged, so no new single-substep bound is introduced.
# Seeds, the first ones tried: 501 (general and what is built on it), 511 (shared), 521 (stack), 531 (coefficients).
FRAMES = 8
EXACT_H = 2.0 ** -10
SLEEP_ES = np.array([0.0, 0.4, 0.8])
CAPS = np.array([np.inf, 0.5, 2.0, 8.0])
COM = (0.3, -0.2, 0.1)
CHAIN_SUBSTEPS = (2, 3)
# 8 x the largest normalised error of the f64 chain against the longdouble chain over the chained scenes, per S (filled in from
# the CPU run, test_the_f64_chain_stays_within_the_recorded_chain_bound prints the figures)
K_SLEEP_CHAIN = {2: 346.0, 3: 509.0}            # 8 x 43.23 (general-h240) and 8 x 63.58 (general-h1200)


def weigh(body, factor, inertia=(1.0, 1.0, 1.0)):
    """The body `factor` times as heavy, its principal inertias scaled by `inertia` as well."""
    body[0] /= factor
    body[1:10] = (body[1:10].reshape(3, 3) / factor / np.asarray(inertia)[:, None]).reshape(-1)
    if body[12]:
        body[12] = -G / body[0]
    return body


def at_rest(body):
    body[22:28] = 0.0
    return body


# ---- (a) general --------------------------------------------------------------------------------------------------------------
# (sleeper shape, where, gravity, mass factor, probes' shapes)
UNITS = ((CUBE, "air", True, 3.0, (CUBE, TETRA)), (HULL16, "air", False, 1.0, (ICOSA, CUBE)), (HULL18, "air", True, 0.5, (HULL16, TETRA)),
         (CUBE, "ground", True, 1.0, (ICOSA, HULL18)), (CUBE, "air", False, 0.2, (CUBE, CUBE)), (ICOSA, "air", True, 2.0, (CUBE, HULL18)),
         (TETRA, "ground", True, 1.0, (CUBE,)), (HULL16, "air", True, 4.0, (TETRA, ICOSA)))
PROBE_MASSES = (0.5, 1.0, 2.0, 4.0)


def scene_general(h, frame, seed=501):
    rng = np.random.default_rng(seed * 1000 + frame)
    bodies, sid, labels, asleep = [], [], [], []
    for k, (shape, where, gravity, mass, probes) in enumerate(UNITS):
        at = np.array([6.0 * (k % 4), 6.0 * (k // 4), 6.0])
        s = pc.new_body(shape, at, pc.random_rotation(rng), gravity=gravity)
        if k == 0:
            s[28:31] = COM
            weigh(s, mass, (1.0, 2.0, 4.0))
        else:
            weigh(s, mass)
        if where == "ground":                                  # a tenth of a millimetre in the ground: a contact mask to keep
            bc.settle(s, shape, -1e-4)
        bodies.append(s), sid.append(shape), labels.append("sleeper"), asleep.append(True)
        for j, probe in enumerate(probes):
            p = pc.new_body(probe, at, pc.random_rotation(rng), spin=bc.spin(rng), gravity=(k + j) % 2 == 0)
            weigh(p, PROBE_MASSES[(k + 2 * j) % 4])
            if j == 0:
                direction = (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0)
            else:
                phi = rng.uniform(0, 2 * np.pi)
                direction = (np.cos(phi), np.sin(phi), rng.uniform(0.0, 0.3))
            bc.approach(rng, s, shape, p, probe, direction, h)
            bodies.append(p), sid.append(probe), labels.append("on" if j == 0 else "beside"), asleep.append(False)
    n = len(bodies)
    return {"bodies": np.array(bodies), "sid": np.array(sid, dtype=np.uint32), "labels": np.array(labels),
            "asleep": np.array(asleep), "e": np.zeros(n), "mu": np.full(n, np.inf), "exact": (), "ground_e": 0.0}


# ---- (b) shared ---------------------------------------------------------------------------------------------------------------
SHARED_SHAPES = (CUBE, ICOSA, HULL16, CUBE, TETRA, HULL18)


def lowest(body, sid):
    return bc.world_vertices(body, sid)[:, 2].min()


def scene_shared(h, frame, seed=511):
    """Per unit: a probe P that comes down on the ground and sideways onto a sleeper S, and an awake body A that runs into P."""
    rng = np.random.default_rng(seed * 1000 + frame)
    bodies, sid, labels, asleep = [], [], [], []
    for k, shape in enumerate(SHARED_SHAPES):
        at = np.array([7.0 * (k % 3), 7.0 * (k // 3), 1.0])
        vz = rng.uniform(0.5, 3.0)
        p = pc.new_body(shape, at, pc.random_rotation(rng), spin=bc.spin(rng))
        bc.settle(p, shape, 0.0)
        other = SHARED_SHAPES[(k + 1) % len(SHARED_SHAPES)]
        s = pc.new_body(other, at, pc.random_rotation(rng))
        for rise in (0.4, 0.8, 1.5, 3.0):                      # the sleeper clear of the ground
            d = np.array([1.0, rng.uniform(-0.2, 0.2), rise])
            d /= np.linalg.norm(d)
            pc.touch(p, shape, s, other, d, 0.0)
            if lowest(s, other) > 0.01:
                break
        closing = rng.uniform(0.5, 2.0)                        # towards the sleeper along d, and vz down
        p[22:25] = d * (closing + vz * d[2]) + np.array([0.0, 0.0, -vz])
        bc.settle(p, shape, rng.uniform(0.2, 0.8) * max(-p[24], 0.0) * h)
        pc.touch(p, shape, s, other, d, 0.0)
        s[31:34] += d * rng.uniform(0.2, 0.8) * closing * h
        a = pc.new_body(CUBE, at, pc.random_rotation(rng), spin=bc.spin(rng))
        bc.approach(rng, p, shape, a, CUBE, (-1.0, rng.uniform(-0.2, 0.2), 0.6), h)
        bodies += [p, at_rest(s), a]
        sid += [shape, other, CUBE]
        labels += ["probe", "sleeper", "awake"]
        asleep += [False, True, False]
    n = len(bodies)
    return {"bodies": np.array(bodies), "sid": np.array(sid, dtype=np.uint32), "labels": np.array(labels),
            "asleep": np.array(asleep), "e": np.zeros(n), "mu": np.full(n, np.inf), "exact": (), "ground_e": 0.0}


# ---- (c) stack ----------------------------------------------------------------------------------------------------------------
STACK_OVERLAP = 2.0 ** -12         # the boxes of a stack stand this deep in each other and in the slab: they touch, one island


def scene_stack(h, frame, seed=521):
    rng = np.random.default_rng(seed * 1000 + frame)
    bodies, sid, labels, asleep = [], [], [], []
    for unit in range(3):
        x = 16.0 * unit
        bodies.append(pc.new_body(SLAB, (x - 1.5, -1.5, 0.5), static=True))      # a shape's vertices span [0, edge]^3 from its position
        sid.append(SLAB), labels.append("slab"), asleep.append(False)
        boxes = [pc.new_body(CUBE, (x, 0.0, 4.5 + k - (k + 1) * STACK_OVERLAP)) for k in range(3)]
        boxes[1] = weigh(boxes[1], 2.0)
        top = pc.new_body(CUBE, (x, 0.0, 9.0), jc.tilt(rng, 0.1), spin=bc.spin(rng, 0.5))
        bc.approach(rng, boxes[2], CUBE, top, CUBE, (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 1.0), h)
        shape = (TETRA, ICOSA, HULL16)[unit]
        side = pc.new_body(shape, (x, 0.0, 5.5), pc.random_rotation(rng), spin=bc.spin(rng), gravity=False)
        bc.approach(rng, boxes[1], CUBE, side, shape, (1.0, rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)), h)
        bodies += boxes + [top, side]
        sid += [CUBE] * 4 + [shape]
        labels += ["stack"] * 3 + ["top", "side"]
        asleep += [True] * 3 + [False] * 2
    n = len(bodies)
    return {"bodies": np.array(bodies), "sid": np.array(sid, dtype=np.uint32), "labels": np.array(labels),
            "asleep": np.array(asleep), "e": np.zeros(n), "mu": np.full(n, np.inf), "exact": (), "ground_e": 0.0}


# ---- (d) materials, (e) bouncing, (f) damped ------------------------------------------------------------------------------------
def coefficients(n, values, seed=531):
    return values[np.random.default_rng(seed).integers(0, len(values), n)]


def scene_materials(h, frame):
    s = scene_general(h, frame)
    return dict(s, mu=coefficients(len(s["sid"]), MUS))


def bouncing(builder):
    def scene(h, frame):
        s = builder(h, frame)
        return dict(s, e=coefficients(len(s["sid"]), SLEEP_ES), ground_e=bc.GROUND_E)
    return scene


def scene_damped(h, frame):
    s = scene_general(h, frame)
    n = len(s["sid"])
    rows = dcs.drag_rows(n, 201)
    rows["max_linear_speed"], rows["max_angular_speed"] = coefficients(n, CAPS, 541), coefficients(n, CAPS, 551)
    return dict(s, rows=rows)


# ---- (g) exact ----------------------------------------------------------------------------------------------------------------
# (sleeper, probe) of each case, and the lone twin of the last probe
EXACT_EQUAL, EXACT_HEAVY, EXACT_TOUCH, EXACT_LONE = (0, 1), (2, 3), (4, 5), 6
EXACT_DEPTH = 2.0 ** -8
EXACT_LONE_SHIFT = 64.0


def scene_exact(h, frame):
    """Unit boxes, identity rotations, no gravity, 8 m up.  EQUAL: a box at rest EXACT_DEPTH deep in a sleeper of its own mass
    properties.  HEAVY: the same on a sleeper 1024 times as heavy.  TOUCH: a box whose lower face lies exactly in the sleeper's
    upper face (SAT value 0: no contact), sliding along it, and LONE: the same box EXACT_LONE_SHIFT m further in x with nothing
    under it.  Every frame moves the cases by 2^-3 m in y."""
    y = frame * 2.0 ** -3
    kw = {"gravity": False}
    bodies = [pc.new_body(CUBE, (0.0, y, 8.0), **kw), pc.new_body(CUBE, (0.0, y, 9.0 - EXACT_DEPTH), **kw),
              weigh(pc.new_body(CUBE, (8.0, y, 8.0), **kw), 1024.0), pc.new_body(CUBE, (8.0, y, 9.0 - EXACT_DEPTH), **kw),
              pc.new_body(CUBE, (16.0, y, 8.0), **kw), pc.new_body(CUBE, (16.0, y, 9.0), velocity=(0.25, 0.0, 0.0), **kw),
              pc.new_body(CUBE, (16.0 + EXACT_LONE_SHIFT, y, 9.0), velocity=(0.25, 0.0, 0.0), **kw)]
    n = len(bodies)
    return {"bodies": np.array(bodies), "sid": np.zeros(n, dtype=np.uint32),
            "labels": np.array(["sleeper", "equal", "sleeper", "heavy", "sleeper", "touch", "lone"]),
            "asleep": np.array([True, False, True, False, True, False, False]), "e": np.zeros(n), "mu": np.full(n, np.inf),
            "exact": tuple(range(n)), "ground_e": 0.0}


# name -> (builder(h, frame), h, friction?, depenetration limit)
def _scenes():
    out = {}
    for h in HS:
        tag = "h%d" % round(1.0 / h)
        out["general-" + tag] = (scene_general, h, False, 0.0)
        out["shared-" + tag] = (scene_shared, h, False, 0.0)
        out["stack-" + tag] = (scene_stack, h, False, 0.0)
        out["materials0-" + tag] = (scene_materials, h, True, 0.0)
        out["materials3-" + tag] = (scene_materials, h, True, 3.0)
        out["bouncing-" + tag] = (bouncing(scene_general), h, False, 0.0)
        out["bouncing-stack-" + tag] = (bouncing(scene_stack), h, False, 0.0)
        out["damped-" + tag] = (scene_damped, h, False, 0.0)
    out["exact-h1024"] = (scene_exact, EXACT_H, False, 0.0)
    return out


SCENES = _scenes()
CHAINED = [n for n in SCENES if n.startswith(("general", "stack", "bouncing"))]


def is_bouncing(name):
    return name.startswith("bouncing")


@functools.lru_cache(maxsize=None)
def build(name, frame):
    builder, h, friction, speed = SCENES[name]
    s = dcs.finish(builder(h, frame), h, friction)
    if not is_bouncing(name):
        s.update(e=None, ground_e=0.0, threshold=0.0)
    s["speed"] = speed
    s["probes"] = ~s["asleep"] & ~dcs.is_fixed(s)
    assert not s["bodies"][s["asleep"], 22:28].any()
    return s


def evaluate(s, state=None, num=None, mutation=None, tau=0.0, manifolds=None, asleep="scene", contact_mask=None):
    """The model's substep of a finished scene (from `state` if given); asleep: the scene's set, or None: everybody awake."""
    return pm.substep(s["bodies"] if state is None else state, pc.table()[1], s["sid"], s["h"], manifolds, s["mu"], s["ground_mu"],
                      s["speed"], num=num, mutation=mutation, tau=tau, restitution=s["e"], ground_restitution=s["ground_e"],
                      bounce_threshold=s["threshold"], damping=s["rows"], asleep=s["asleep"] if isinstance(asleep, str) else asleep,
                      contact_mask=contact_mask)


def errors(s, got, res, start=None):
    return xk.scene_errors(s, got, res, s["bodies"] if start is None else start)          # no joints: the links are the manifolds


def excluded(res, s):
    """xprec_damping_cases.excluded unchanged; the sleeping reading has no branch of its own: a sleeper takes part or it does not
    by the asleep set, which is given."""
    return dcs.excluded(res, s)


bounds = bc.bounds


def carries(res):
    """The body-substeps the second cap and the floor count: awake bodies with a pair point whose other end is asleep."""
    return (res["n_sleeper_points"] > 0) & ~res["asleep"]


def caps_floor(name):
    """xprec_check.assert_caps' floor: the exact scene, asserted by name, has none."""
    return 0 if name.startswith("exact") else 20


def frame_result(s, start, seed):
    """The longdouble model's result of the scene's substep from `start`, with its one-ulp sensitivity."""
    return xk.model_frame(s, functools.partial(evaluate, s), start, seed, s["exact"], want=False)[0]


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """Returns dict(h=, frames=[(start, want, res, scene)]): `want` the f64 evaluation's state after the substep, res the
    longdouble model's result from `start` with its one-ulp sensitivity, scene = build(name, f)."""
    out = []
    for f in range(FRAMES):
        s = build(name, f)
        res, want = xk.model_frame(s, functools.partial(evaluate, s), s["bodies"], f, s["exact"])
        out.append((s["bodies"], want, res, s))
    return {"h": SCENES[name][1], "frames": out}


def check_states(name, got_states):
    """got_states[f]: the state after frame f of an implementation under test.  Asserts bounds() on every body-substep that is
    not excluded -- a sleeper's model state is its input, so a sleeper is held to it as well; returns (normalised errors,
    excluded, carries), each a list over frames of (n,) arrays."""
    frames = [(start, res, s) for start, _, res, s in trajectory(name)["frames"]]
    return xk.check_frames(name, frames, got_states, errors=xk.scene_errors, excluded=excluded, bound=bounds,
                           carries=lambda res, s: carries(res))


# ---- GJK + EPA ------------------------------------------------------------------------------------------------------------------
def gjk_result(s, start):
    """Stage S on the manifolds of a GJK + EPA substep as xprec_pairs_cases.gjk_manifolds_of can reproduce them, from the model's own
    post-integrate frames -- a sleeper's is Rigid::frame() of its stored pose -- for every pair the model's stage N looks at.
    Returns (result, excluded: the model's and the bodies with a pair that cannot be reproduced, the bodies that touch a pair)."""
    num = xm.native()
    sat = evaluate(s, state=start)
    frames = [(num.to_f64(p), num.to_f64(q)) for p, q in sat["frames"]]
    shapes = pc.table()[1]
    n = len(start)
    inert = s["asleep"] | dcs.is_fixed(s)
    centre = [np.asarray(xm.frame_apply(frames[b][0], frames[b][1], shapes[int(s["sid"][b])]["centroid"])) for b in range(n)]
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if not (inert[i] and inert[j])
             and np.linalg.norm(centre[i] - centre[j]) <= shapes[int(s["sid"][i])]["radius"] + shapes[int(s["sid"][j])]["radius"] + 1e-3]
    manifolds, unknown, touching = pc.gjk_manifolds_of(frames, pairs, s["sid"])
    res = evaluate(s, state=start, manifolds=manifolds, tau=TAU)
    x = excluded(res, s)
    x[sorted(unknown)] = True
    mask = np.zeros(n, dtype=bool)
    mask[sorted(touching)] = True
    return res, x, mask


# ---- frames of S substeps -------------------------------------------------------------------------------------------------------
def chain(s, start, substeps, num=None, mutation_at=None):
    """The model chained S times from `start` with the sleepers frozen (the asleep set does not change within a frame), the
    state carried in the model's scalars.  mutation_at: {substep: mutation}.  Returns (the last substep's result, excluded: a body
    excluded in any substep, carries: a sleeper's point in any substep, every pair that touched)."""
    state = start
    n = len(start)
    x, c, links = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), set()
    for k in range(substeps):
        res = evaluate(s, state=state, num=num, tau=TAU, mutation=(mutation_at or {}).get(k))
        x |= excluded(res, s)
        c |= carries(res)
        links |= set(res["manifolds"])
        state = res["state"]
    return res, x, c, sorted(links)


def chain_errors(s, got, res, start, links, substeps):
    """Normalised as a single substep's, with the frame's h = dt / S in the velocities."""
    return pc.normalized_errors(got, res["state"], start, s["ext"], s["h"], links)
