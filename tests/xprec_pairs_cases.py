"""The body-body contact scenes shared by test_xprec_pairs_oracle.py (oracle vs model, CPU) and test_gpu_xprec_pairs.py (HIP
vs oracle and model): the scenes, the oracle's trajectory of each as a sequence of SINGLE-SUBSTEP frames (dt = h,
substeps = 1), the model (tests/xprec_pairs_model.py) re-seeded from the oracle's state before every one, the bound and
the exclusions.

Bound.  The form of xprec_cases (K S eps scale with S = 1), `scale` = |x| + extent of the body or of the largest body it
touches in the substep, whichever is larger.  Manifold quantities (separation, points) are bound by K_MANIFOLD eps scale,
scale = the larger |frame position| + extent of the pair.

Scenes.  (a) pairs in general position from every shape class, (b) exactly aligned boxes with binary-exact poses, (c) cubes
crossed edge over edge, (d) the categories of edge_rigids in touching pairs, (e) a 40-body pile on the ground with mixed
friction and the depenetration limit.  A polytope record holds 32 faces and 64 edges, a hull of 18 vertices at most (32
faces, 48 edges); that hull reaches the widest kernels, as in test_gpu_pairs.py."""
import ctypes as C
import functools

import numpy as np

import edge_rigids as er
import hull_util as hu
import material_model as mm
import oracle_binding as ob
import xprec_cases as xc
import xprec_model as xm
import xprec_pairs_model as pm
from xprec_cases import COND_MIN, EPS, FLIP_MIN, SENSITIVITY_MAX, TAU

PAD = 0.02
G = 9.81
CUBE, TETRA, ICOSA, HULL16, HULL18, SLAB, EDGE_HULL = range(7)
NO_JOINTS = np.zeros(0, dtype=np.dtype([("raw", np.uint8, C.sizeof(ob.Joint))]))
MUS = np.array([0.0, 0.2, 0.5, 1.0, np.inf])                   # test_gpu_materials.MUS
GROUND_MU = 0.4
HS = (1.0 / 1200.0, 1.0 / 240.0)
# Measured with the oracle against the longdouble model (tests/test_xprec_pairs_oracle.py prints them), largest normalised
# error of a checked body-substep per scene, stage S o N (in brackets: stage S on the oracle's manifolds):
#   general  h 1/1200: 32.0 (29.6)   h 1/240: 12.2 (10.9)      aligned  h 1/1200: 0.6 (0.6)    h 1/240: 0.7 (0.7)
#   crossed  h 1/1200:  6.6 ( 6.6)   h 1/240: 11.0 (11.0)      edge     h 1/1200: 21.8 (22.8)  h 1/240: 81.9 (81.9)
#   pile h 1/1200 plain: 51.2 (24.3)   pile h 1/240 friction: 6.3 (7.0)   pile h 1/240 friction, limit 3 m/s: 7.9 (6.9)
# 99 % of the body-substeps of every scene stay below 17.  The maximum is a body of asymmetric inverse inertia.  K_PAIRS
# is 8x the largest value (xprec_cases.K's margin).  The 40-digit mpmath model moves the substep that holds the maximum of scenes
# (b) and (d) by 0.004 in these units at most (test_longdouble_model_equals_mpmath_model): longdouble's rounding sets none.
K_PAIRS = 656.0
# Manifolds, normalised error of separation and points of a checked touching pair: general 4.1, aligned 0 (exact), crossed
# 0.9, edge 2.1, pile 10.3 / 7.2 / 13.6 (a clipped point where the incident edge meets the side plane at a flat angle);
# 2 000 random pairs: 6.8.  K_MANIFOLD is 8x the largest.
K_MANIFOLD = 109.0


@functools.lru_cache(maxsize=None)
def table():
    """The shape table of every scene: oracle Polytope array, the model's shapes, and the hulls' raw arrays."""
    h16, h18 = hu.random_hull(1), hu.random_hull(7, 18, 0.6)
    ev, ec, et = er.shapes()
    edge_hull = (ev[er.HULL16], et[er.HULL16][0], et[er.HULL16][1], ec[er.HULL16])
    polys = (ob.Polytope * 7)(ob.polytope("cube"), ob.polytope("tetrahedron", 0.5), ob.polytope("icosahedron", 0.5),
                              hu.as_oracle(*h16), hu.as_oracle(*h18), ob.polytope("cube", 4.0), hu.as_oracle(*edge_hull))
    return polys, [pm.shape(p) for p in polys], {HULL16: h16, HULL18: h18, EDGE_HULL: edge_hull}


def capi_polytopes(capi):
    _, _, hulls = table()
    return [capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_TETRAHEDRON, 0.5), capi.polytope(capi.SHAPE_ICOSAHEDRON, 0.5),
            hu.as_capi(*hulls[HULL16]), hu.as_capi(*hulls[HULL18]), capi.polytope(capi.SHAPE_CUBE, 4.0), hu.as_capi(*hulls[EDGE_HULL])]


def new_body(sid, position, rotation=(1.0, 0.0, 0.0, 0.0), velocity=(0, 0, 0), spin=(0, 0, 0), gravity=True, static=False):
    """Rigid::new of the shape at density 1 (rigid.rs:43-73), placed; a static body has inverse mass and inertia 0.  A hull
    takes the cube's mass and inertia about its own centroid."""
    L, polys = ob.load(), table()[0]
    m, r = ob.Metrics(), ob.Rigid()
    hull = sid in (HULL16, HULL18, EDGE_HULL)     # their faces are not wound consistently: the unit cube's mass properties
    L.o_rigid_metrics(C.byref(polys[CUBE if hull else sid]), 1.0, C.byref(m))
    assert L.o_rigid_new(C.byref(m), C.byref(r)) == 1
    b = r.np()
    if hull:
        b[28:31] = polys[sid].centroid.np()
    b[10:22] = 0.0
    if static:
        b[0:10] = 0.0
    elif gravity:
        b[12] = -G / b[0]
    b[22:25], b[25:28], b[31:34], b[34:38] = velocity, spin, position, rotation
    return b


def frames_of(bodies):
    L = ob.load()
    out = []
    for b in bodies:
        f = L.o_rigid_frame(C.byref(ob.Rigid.from_np(b)))
        out.append((f.position.np(), f.rotation.np()))
    return out


def touch(a, sid_a, b, sid_b, direction, depth):
    """Move body b along `direction` from body a's position until the pair's separation is -depth (bisection on the
    oracle's SAT: placement only, nothing is asserted from it)."""
    polys = table()[0]
    direction = np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction)
    base = a[31:34] + a[28:31] - b[28:31]
    lo, hi = 0.0, 8.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        b[31:34] = base + direction * mid
        fa, fb = frames_of([a, b])
        m = ob.sat(fa, fb, polys[sid_a], polys[sid_b])
        if m.separated or m.separation > -depth:
            hi = mid
        else:
            lo = mid
    b[31:34] = base + direction * hi
    return b


def random_rotation(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def scene_general(seed=11):
    """(a) every shape class, pairs in general position: the pair approaches at 0.2 to 1 m/s from 0 to 3 mm apart or starts
    up to 3 cm deep, so that contacts begin at different substeps; 4 m between pairs, no ground in reach."""
    rng = np.random.default_rng(seed)
    classes = [(CUBE, CUBE), (CUBE, TETRA), (CUBE, ICOSA), (TETRA, ICOSA), (ICOSA, ICOSA), (HULL16, HULL16), (HULL18, CUBE),
               (HULL18, HULL16)]
    bodies, sid, labels = [], [], []
    for k, (sa, sb) in enumerate(classes * 4):
        at = np.array([4.0 * (k % 8), 4.0 * (k // 8), 6.0])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        a = new_body(sa, at, random_rotation(rng), spin=rng.uniform(-2, 2, 3), gravity=k % 2 == 0)
        b = new_body(sb, at, random_rotation(rng), spin=rng.uniform(-2, 2, 3), gravity=k % 2 == 0)
        depth = rng.uniform(0.001, 0.03) if k % 3 else -rng.uniform(0.0, 0.003)
        touch(a, sa, b, sb, d, depth)
        b[22:25] = -d * rng.uniform(0.2, 1.0)
        bodies += [a, b]
        sid += [sa, sb]
        labels += ["%d-%d" % (sa, sb)] * 2
    return np.array(bodies), np.array(sid, dtype=np.uint32), np.array(labels)


def scene_aligned(frame=0):
    """(b) binary-exact poses, identity rotations, at rest and without forces, so that the post-integrate frames are exact
    in f64 and in the model alike and every tie is decided by the stated rule: a 6-box column, a box resting corner over
    centre on another, a box on two boxes.  Every frame of the scene is a fresh exact configuration (the depth and the
    lateral offsets change with the frame): the oracle's own next state is no longer exact."""
    d = 2.0 ** -(6 + frame % 5)
    s = (frame % 4) * 2.0 ** -4
    z0 = 3.0 + frame * 2.0 ** -3
    kw = {"gravity": False}
    bodies = [new_body(CUBE, (0.0, 0.0, z0 + k * (1.0 - d)), **kw) for k in range(6)]
    bodies += [new_body(CUBE, (4.0, 0.0, z0), **kw), new_body(CUBE, (4.5 + s, 0.5 - s, z0 + 1.0 - d), **kw)]
    bodies += [new_body(CUBE, (8.0, 0.0, z0), **kw), new_body(CUBE, (9.25, s, z0), **kw), new_body(CUBE, (8.625, 0.0, z0 + 1.0 - d), **kw)]
    labels = ["column"] * 6 + ["corner"] * 2 + ["bridge"] * 3
    return np.array(bodies), np.zeros(len(bodies), dtype=np.uint32), np.array(labels)


def scene_crossed(seed=5):
    """(c) edge-edge: a cube turned 45 degrees about y, edge up, under a cube turned 45 degrees about x, edge down, the
    upper one yawed by a few degrees and sinking at 0.1 to 0.4 m/s; gravity off."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(np.pi / 8), np.sin(np.pi / 8)
    bodies = []
    for k in range(6):
        at = np.array([4.0 * k, 0.0, 5.0])
        yaw = rng.uniform(-0.3, 0.3)
        qz = np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
        qx = np.array([c, s, 0.0, 0.0])
        upper_q = np.array(xm.qmul(qz[:, None], qx[:, None]))[:, 0]
        a = new_body(CUBE, at, (c, 0.0, s, 0.0), gravity=False)
        b = new_body(CUBE, at, upper_q, gravity=False)
        touch(a, CUBE, b, CUBE, (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 1.0), rng.uniform(0.002, 0.02))
        b[24] = -rng.uniform(0.1, 0.4)
        bodies += [a, b]
    return np.array(bodies), np.zeros(len(bodies), dtype=np.uint32), np.array(["crossed"] * len(bodies))


EDGE_CATEGORIES = ("asym_inertia", "com_offset", "static_linear", "mass_extreme", "far", "spin")
EDGE_SHAPES = {er.CUBE: CUBE, er.TETRA: TETRA, er.ICOSA: ICOSA, er.HULL16: EDGE_HULL}


def scene_edge(h, seed=21):
    """(d) the categories of edge_rigids (asymmetric inertia, offset centre of mass, inverse mass 0, inverse mass 1e-6 and
    1e6, |x| = 1e4 m, h |w| / 2 near 1; three bodies each, as generate makes them, near the ground), each touched by an
    ordinary box 1 to 20 mm deep from the side or above; and two boxes on a static slab (inverse mass 0)."""
    rng = np.random.default_rng(seed)
    edge, esid, _, _, elabels = er.generate(seed, 3, h=h)
    bodies, sid, labels = [], [], []
    for cat in EDGE_CATEGORIES:
        for k in np.nonzero(elabels == cat)[0]:
            a, sa = edge[k].copy(), EDGE_SHAPES[int(esid[k])]
            b = new_body(CUBE, a[31:34], random_rotation(rng), velocity=rng.uniform(-0.3, 0.3, 3), spin=rng.uniform(-2, 2, 3))
            d = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.3, 1.0)])
            touch(a, sa, b, CUBE, d, rng.uniform(0.001, 0.02))
            bodies += [a, b]
            sid += [sa, CUBE]
            labels += [cat] * 2
    for k in range(2):
        slab = new_body(SLAB, (40.0 + 8.0 * k, 40.0, -3.5), static=True)
        box = new_body(CUBE, slab[31:34], random_rotation(rng) if k else (1.0, 0.0, 0.0, 0.0), velocity=(0.2, 0.1, -0.2))
        touch(slab, SLAB, box, CUBE, (0.05 * k, 0.0, 1.0), 2.0 ** -9)
        bodies += [slab, box]
        sid += [SLAB, CUBE]
        labels += ["slab"] * 2
    return np.array(bodies), np.array(sid, dtype=np.uint32), np.array(labels)


def scene_pile(seed=3):
    """(e) 40 bodies of the three reference shapes dropped into a 2.2 m wide heap on the ground."""
    rng = np.random.default_rng(seed)
    bodies, sid = [], []
    for k in range(40):
        s = (CUBE, TETRA, ICOSA)[k % 3]
        at = (rng.uniform(0, 2.2), rng.uniform(0, 2.2), rng.uniform(0.1, 2.6))
        bodies.append(new_body(s, at, random_rotation(rng), velocity=rng.uniform(-0.3, 0.3, 3), spin=rng.uniform(-1, 1, 3)))
        sid.append(s)
    mu = MUS[rng.integers(0, len(MUS), 40)]
    return np.array(bodies), np.array(sid, dtype=np.uint32), np.array(["pile"] * 40), mu


# name -> (builder of (bodies, sid, labels), h, substeps, materials (mu, ground_mu) or None, depenetration speed)
def _scenes():
    out = {}
    for hi, h in enumerate(HS):
        tag = "h%d" % round(1.0 / h)
        out["general-" + tag] = (scene_general, h, 24, None, 0.0)
        out["aligned-" + tag] = (scene_aligned, h, 20, None, 0.0)
        out["crossed-" + tag] = (scene_crossed, h, 24, None, 0.0)
        out["edge-" + tag] = (functools.partial(scene_edge, h), h, 20, None, 0.0)
    out["pile-h1200-plain"] = (scene_pile, HS[0], 20, None, 0.0)
    out["pile-h240-mu"] = (scene_pile, HS[1], 20, "mixed", 0.0)
    out["pile-h240-mu-limit3"] = (scene_pile, HS[1], 20, "mixed", 3.0)
    return out


SCENES = _scenes()


def build(name):
    builder, h, substeps, materials, speed = SCENES[name]
    made = builder()
    bodies, sid, labels = made[:3]
    mu = made[3] if materials and len(made) > 3 else None
    return bodies, sid, labels, h, substeps, mu, (GROUND_MU if mu is not None else np.inf), speed


def start_of(name, f, previous):
    """The state substep f starts from: the oracle's previous result, but for (b) a fresh exact configuration."""
    if SCENES[name][0] is scene_aligned:
        return scene_aligned(f)[0]
    return previous


def oracle_substep(state, sid, h, mu=None, ground_mu=np.inf, speed=0.0, narrowphase=0):
    """One single-substep frame of the f64 definition: op_contacts_* (oracle/xpbd_pairs_oracle.c), or with materials the
    model the device is held to bit for bit (tests/material_model.py, SAT only)."""
    polys = table()[0]
    if mu is None:
        return ob.contacts_step_joints(state, sid, polys, NO_JOINTS, h, 1, PAD, narrowphase=narrowphase, max_depenetration_speed=speed)
    assert narrowphase == 0
    return mm.Model(state, sid, polys, mu, ground_mu, pad=PAD, max_depenetration_speed=speed).step(h, 1).copy()


def oracle_manifolds(state, sid, h):
    """What the oracle's substep sees: its post-integrate frames, its neighbour pairs (broadphase and the tight-sphere
    pre-test, as xpbd_pairs_oracle.h states them) and op_sat of each.  Returns (frames, {(i, j): Manifold}, the integrated
    bodies)."""
    L, (polys, shapes, _) = ob.load(), table()
    off, nb = ob.broadphase(state, sid, polys, h, PAD)
    moved = []
    for b in state:
        r = ob.Rigid.from_np(b)
        L.o_rigid_integrate(C.byref(r), h)
        moved.append(r.np())
    frames = frames_of(moved)
    out = {}
    for i in range(len(state)):
        for j in nb[off[i]:off[i + 1]]:
            j = int(j)
            if j > i:
                out[(i, j)] = ob.sat(frames[i], frames[j], polys[int(sid[i])], polys[int(sid[j])])
    return frames, out, np.array(moved)


def as_model_manifolds(oracle):
    """The oracle's touching manifolds in the form stage S takes."""
    out = {}
    for key, m in oracle.items():
        if not m.separated and m.n_points:
            ref, inc = m.points()
            out[key] = {"separated": False, "feature": int(m.feature), "p_ref": list(ref), "p_inc": list(inc)}
    return out


def extents(sid, bodies):
    shapes = table()[1]
    r = np.array([np.linalg.norm(shapes[int(s)]["verts"], axis=1).max() for s in sid])
    return r + 2 * np.linalg.norm(np.asarray(bodies)[:, 28:31], axis=1)


def scales(start, got, ext, pairs):
    """|x| + extent per body, raised to that of the largest body it touches."""
    x = np.maximum(np.linalg.norm(start[:, 31:34], axis=1), np.linalg.norm(np.asarray(got)[:, 31:34], axis=1))
    scale, own = x + ext, x + ext
    scale = scale.copy()
    for i, j in pairs:
        scale[i], scale[j] = max(scale[i], own[j]), max(scale[j], own[i])
    return scale


def normalized_errors(got, model_state, start, ext, h, pairs):
    """Per body: max over pose fields of |got - model| / (eps scale [/ extent] [/ h]) (xprec_cases.normalized_errors, S = 1)."""
    num = xm.native()
    d = np.abs(num.to_f64(num.conv(got) - model_state))
    scale = scales(start, got, ext, pairs)
    turn = scale / ext
    return np.max(np.stack([d[:, 31:34].max(axis=1) / (EPS * scale), d[:, 34:38].max(axis=1) / (EPS * turn),
                            d[:, 22:25].max(axis=1) * h / (EPS * scale), d[:, 25:28].max(axis=1) * h / (EPS * turn)]), axis=0)


def excluded(res):
    """Body-substeps left out of the pose check: a model margin in (0, TAU] (ground decision, friction or limit branch,
    a manifold decision of one of the body's pairs), |c1 - c0| below COND_MIN, |delta.s| below FLIP_MIN, or a one-ulp
    sensitivity above SENSITIVITY_MAX."""
    n = len(res["mask"])
    x = ((res["margin"] <= TAU) | (res["branch"] <= TAU) | (res["cond"] < COND_MIN) | (res["pair_cond"] < COND_MIN)
         | (res["flip_margin"] < FLIP_MIN) | ~res["domain"])
    if "sensitivity" in res:
        x = x | (res["sensitivity"] > SENSITIVITY_MAX)
    for i, j in res["undecided"]:
        x[i] = x[j] = True
    return x


def compare_manifold(m, o, poly_a, poly_b, scale):
    """A stage N result against an op_manifold-like record `o` (attributes or mapping).  Returns (None or what differs in
    the discrete fields, normalised error of separation and points)."""
    get = (lambda k: o[k]) if not hasattr(o, "separated") else (lambda k: getattr(o, k))
    n_points = int(get("n_points"))
    m_touching = not m["separated"] and len(m["p_ref"]) > 0
    if m_touching != (n_points > 0):
        return "touching: %d points, want %d" % (n_points, len(m["p_ref"])), 0.0
    if not m_touching:
        return None, 0.0
    if m["feature"] != int(get("feature")):
        return "feature %d, want %d" % (int(get("feature")), m["feature"]), 0.0
    if m["feature"] == pm.EDGES:
        ea = frozenset(int(v) for v in poly_a.edges[int(get("index_a"))])
        eb = frozenset(int(v) for v in poly_b.edges[int(get("index_b"))])
        if (ea, eb) != (m["edge_a"], m["edge_b"]):
            return "supporting edges", 0.0
    elif (int(get("index_a")), int(get("index_b"))) != (m["index_a"], m["index_b"]):
        return "faces (%d, %d), want (%d, %d)" % (int(get("index_a")), int(get("index_b")), m["index_a"], m["index_b"]), 0.0
    if n_points != len(m["p_ref"]):
        return "n_points %d, want %d" % (n_points, len(m["p_ref"])), 0.0
    num = xm.native()
    err = abs(float(num.conv(np.float64(get("separation"))) - m["separation"]))
    for key in ("p_ref", "p_inc"):
        got = num.conv(np.array([[v.x, v.y, v.z] for v in get(key)[:n_points]]) if hasattr(o, "separated")
                       else np.asarray(get(key))[:n_points])
        want = np.stack(m[key])
        d = np.abs(num.to_f64(got[:, None, :] - want[None, :, :])).max(axis=2)        # nearest matching, as sets
        err = max(err, d.min(axis=1).max(), d.min(axis=0).max())
    return None, err / (EPS * scale)


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """The oracle over the scene's single-substep frames and the model stepped from the oracle's state at the start of
    each: stage S o N (`res`, with its one-ulp sensitivity) and stage S on the oracle's manifolds (`given`).
    Returns dict: start, sid, labels, ext, h, mu, ground_mu, speed and frames [(start state, oracle state, oracle frames,
    oracle manifolds, res, given, integrated bodies)]."""
    bodies, sid, labels, h, substeps, mu, ground_mu, speed = build(name)
    shapes = table()[1]
    ext = extents(sid, bodies)
    state, out = bodies, []
    for f in range(substeps):
        state = start_of(name, f, state)
        want = oracle_substep(state, sid, h, mu, ground_mu, speed)
        frames, manifolds, integrated = oracle_manifolds(state, sid, h)
        res = pm.substep(state, shapes, sid, h, None, mu, ground_mu, speed, tau=TAU)
        given = pm.substep(state, shapes, sid, h, as_model_manifolds(manifolds), mu, ground_mu, speed)
        pairs = list(res["manifolds"])
        if SCENES[name][0] is scene_aligned:
            # an exact tie is decided by the stated rule; one ulp beside it the decision is another one, by construction
            res["sensitivity"] = np.zeros(len(state))
        else:
            moved = pm.substep(xc.nudged(state, f), shapes, sid, h, None, mu, ground_mu, speed)
            res["sensitivity"] = normalized_errors(xm.native().to_f64(moved["state"]), res["state"], state, ext, h, pairs)
        out.append((state, want, frames, manifolds, res, given, integrated))
        state = want
    return {"start": bodies, "sid": sid, "labels": labels, "ext": ext, "h": h, "mu": mu, "ground_mu": ground_mu, "speed": speed,
            "frames": out}


def check_states(name, got_states, which="res", k=None, model=None):
    """got_states[f]: the state after substep f of an implementation under test.  Asserts the bound on every body-substep
    that is not excluded; returns (normalised errors, excluded) (frames, n).  `model`: per-frame model results to use
    instead of the trajectory's (the mutation check)."""
    t = trajectory(name)
    k = K_PAIRS if k is None else k
    errs, excl = [], []
    for f, (start, _, _, _, res, given, _) in enumerate(t["frames"]):
        m = model[f] if model is not None else (res if which == "res" else given)
        e = normalized_errors(got_states[f], m["state"], start, t["ext"], t["h"], list(res["manifolds"]))
        x = excluded(res)
        bad = np.nonzero(~x & ~(e <= k))[0]
        assert not len(bad), "%s substep %d: bodies %s (%s) beyond K = %g: %s" % (name, f, bad[:8], t["labels"][bad[:8]], k, e[bad[:8]])
        errs.append(e)
        excl.append(x)
    return np.array(errs), np.array(excl)


# ---- GJK + EPA narrowphase ------------------------------------------------------------------------------------------------
# xpbd_pairs_oracle.c, gjk_manifold: the face most aligned with EPA's normal (cosine >= 0.999, A on ties) is the reference
# face of a clip as in the SAT; otherwise, or when the clip leaves nothing, the one EPA point with A as reference body.
FACE_ALIGN = 0.999
# EPA ends on a face of the Minkowski difference: depth and normal carry the f64 rounding of that face's plane (below 1e-12
# for edges of 0.1 to 1 m), and its two points are depth * normal apart.  The normal is compared where the model's best
# axis leads every other axis by AXIS_UNIQUE metres.
EPA_DEPTH_TOL, EPA_NORMAL_TOL, AXIS_UNIQUE = 1e-9, 1e-9, 1e-6


def gjk_model_manifolds(state, sid, h):
    """The manifolds of a GJK + EPA substep as the model can reproduce them, for the oracle's neighbour pairs: stage N's own
    face clip where its largest query is a face axis (EPA's normal is then that face's), or EPA's point pair after its depth
    and normal have been checked against stage N's largest query where that is an edge axis no face is aligned with.
    Returns ({(i, j): manifold}, the bodies with a pair the model cannot reproduce, the bodies that touch a pair)."""
    frames, oman, _ = oracle_manifolds(state, sid, h)
    return gjk_manifolds_of(frames, oman, sid)


def gjk_manifolds_of(frames, pairs, sid):
    """gjk_model_manifolds on given f64 frames [(position, rotation)] and pairs (i, j), i < j: for a caller whose frames are not
    every body's integrated pose."""
    polys, shapes, _ = table()
    oman = pairs
    num = xm.native()
    out, unknown, touching = {}, set(), set()
    for i, j in oman:
        pa, pb = polys[int(sid[i])], polys[int(sid[j])]
        r, _ = ob.gjk_epa_cached(frames[i], frames[j], pa, pb, np.zeros(3))
        m = pm.manifold(frames[i], frames[j], shapes[int(sid[i])], shapes[int(sid[j])])
        if m["margins"]["touch"] <= 1e-7 or r.status == ob.GJK_DEGENERATE:
            unknown |= {i, j}
            continue
        assert (r.status == ob.GJK_PENETRATING) == (not m["separated"]), (i, j, m["margins"])
        if m["separated"]:
            continue
        touching |= {i, j}
        assert abs(r.depth - float(m["depth"])) <= EPA_DEPTH_TOL, (i, j, r.depth, float(m["depth"]))
        if m["margins"]["axis"] <= AXIS_UNIQUE or not pm.decided(m, TAU):
            unknown |= {i, j}
            continue
        axis = num.to_f64(m["axis"])
        assert np.abs(r.normal.np() - axis).max() <= EPA_NORMAL_TOL, (i, j, r.normal.np(), axis)
        a, b, e = m["query"]
        cos_a, cos_b = (axis @ m["face_axes"][0]).max(), (axis @ m["face_axes"][1]).max()
        if e is None or e <= max(a, b):                       # a face axis: cosine 1 on its own body
            tie = (cos_b if a >= b else cos_a) >= 1 - 1e-9    # an exactly opposed face of the other body: A on ties
            if tie and a < b:
                unknown |= {i, j}                             # the SAT's reference face is B's, this rule's is A's
            elif m["p_ref"]:
                out[(i, j)] = m
            else:
                unknown |= {i, j}
        elif max(cos_a, cos_b) >= FACE_ALIGN - 1e-6:
            unknown |= {i, j}                                 # an edge axis within the alignment cone of a face: that face's clip
        else:
            p_a, p_b = r.point_a.np(), r.point_b.np()
            assert np.abs((p_a - p_b) - r.depth * axis).max() <= 2 * EPA_DEPTH_TOL, (i, j)
            out[(i, j)] = {"separated": False, "feature": pm.EDGES, "p_ref": [p_a], "p_inc": [p_b]}
    return out, unknown, touching


@functools.lru_cache(maxsize=None)
def gjk_trajectory(name):
    """The oracle under OP_NARROWPHASE_GJK_EPA over the scene's single-substep frames (material-free scenes: the materials
    model is SAT only) and stage S on gjk_model_manifolds from the oracle's state at the start of each.
    Returns [(start, oracle state, model result, excluded bodies, bodies touching a pair)]."""
    bodies, sid, labels, h, substeps, mu, ground_mu, speed = build(name)
    assert mu is None
    shapes = table()[1]
    state, out = bodies, []
    for f in range(substeps):
        state = start_of(name, f, state)
        want = oracle_substep(state, sid, h, speed=speed, narrowphase=1)
        manifolds, unknown, touching = gjk_model_manifolds(state, sid, h)
        res = pm.substep(state, shapes, sid, h, manifolds, max_depenetration_speed=speed)
        x = excluded(res)
        x[sorted(unknown)] = True
        mask = np.zeros(len(sid), dtype=bool)
        mask[sorted(touching)] = True
        out.append((state, want, res, x, mask))
        state = want
    return out


def check_gjk_states(name, got_states):
    """As check_states for the GJK + EPA trajectory.  Returns (checked, all) body-substeps that touch a pair."""
    t = trajectory(name)
    checked = total = 0
    for f, (start, _, res, x, touching) in enumerate(gjk_trajectory(name)):
        e = normalized_errors(got_states[f], res["state"], start, t["ext"], t["h"], list(res["manifolds"]))
        bad = np.nonzero(~x & ~(e <= K_PAIRS))[0]
        assert not len(bad), "%s GJK substep %d: bodies %s beyond K = %g: %s" % (name, f, bad[:8], K_PAIRS, e[bad[:8]])
        checked, total = checked + int((touching & ~x).sum()), total + int(touching.sum())
    return checked, total
