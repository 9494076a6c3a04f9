"""What the extended-precision families (xprec_joints_cases.py, _drives_, _bounce_, _damping_, _sleep_) share on the CPU side:
the links and the normalised errors of a frame, the check loop with its one assertion message, the exclusion caps, and the
per-frame block of every trajectory (the longdouble result with its one-ulp sensitivity, and the f64 evaluation).  Plain
functions that take the family's callables; scenes, bounds, exclusion rules and `carries` stay with the family.  Imports no
device code.  xprec_pairs_cases.check_states (a `which=` result and an oracle) and xprec_cases.py have contracts of their own."""
import numpy as np

import xprec_cases as xc
import xprec_model as xm
import xprec_pairs_cases as pc
from xprec_cases import TAU


def joint_links(scene, res):
    """The body pairs that act on each other in the substep: touching pairs and joints."""
    return list(res["manifolds"]) + [(int(j["body_a"]), int(j["body_b"])) for j in scene["joints"]]


def scene_errors(scene, got, res, start):
    """xprec_pairs_cases.normalized_errors of `got` against the model's result, with the scene's extents, h and links."""
    return pc.normalized_errors(got, res["state"], start, scene["ext"], scene["h"], joint_links(scene, res))


def in_band(margin):
    """A decision one rounding could turn: the margin within (0, TAU] (exactly 0 is decided by the stated rule)."""
    return (margin > 0) & (margin <= TAU)


def worst(errs, excl):
    """The largest normalised error of a checked body-substep."""
    return max(float(np.where(x, 0, e).max()) for e, x in zip(errs, excl))


def check_frames(name, frames, got_states, *, errors, excluded, bound, carries):
    """frames: (start, res, scene) per frame; got_states[f]: the state after frame f of an implementation under test.  The
    family's errors(scene, got, res, start), excluded(res, scene), bound(res) (a number or one per body) and
    carries(res, scene).  Asserts the bound on every body-substep that is not excluded; returns (normalised errors, excluded,
    carries), each a list over frames of (n,) arrays."""
    errs, excl, entry = [], [], []
    for f, (start, res, scene) in enumerate(frames):
        e = errors(scene, got_states[f], res, start)
        x = excluded(res, scene)
        k = np.broadcast_to(np.asarray(bound(res), dtype=np.float64), e.shape)
        bad = np.nonzero(~x & ~(e <= k))[0]
        assert not len(bad), "%s frame %d: bodies %s (%s) beyond K = %s: %s" % (name, f, bad[:8], scene["labels"][bad[:8]], k[bad[:8]], e[bad[:8]])
        errs.append(e)
        excl.append(x)
        entry.append(carries(res, scene))
    return errs, excl, entry


def assert_caps(name, excl, carries, floor=20):
    """At most 10 % of all body-substeps, and of those that carry what the family checks, are excluded, and at least `floor` of
    the latter are checked."""
    x, c = np.concatenate(excl), np.concatenate(carries)
    assert x.mean() <= 0.10, (name, x.mean())
    assert (x & c).sum() <= 0.10 * c.sum(), (name, (x & c).sum(), c.sum())
    assert (c & ~x).sum() >= floor, (name, (c & ~x).sum())


def nudged(state, seed, exact):
    """xprec_cases.nudged, except on the bodies whose state is binary-exact by construction."""
    out = xc.nudged(state, seed)
    out[list(exact)] = state[list(exact)]
    return out


def model_frame(scene, evaluate, start, seed, exact, *, want=True, nudge_on_res_manifolds=False):
    """One frame of a trajectory.  evaluate(state, **kw) is the family's model substep of `scene`.  Returns (res, want): the
    longdouble model's result from `start` with res["sensitivity"], its normalised move when the start moves by one ulp (on the
    model's own manifolds if asked: that keeps a large scene's brute-force stage N to two), and the f64 evaluation's state
    after the substep (None unless wanted).  exact: the bodies on an exact tie in this frame; there the stated rule decides, one
    ulp beside it the decision is another one, so their sensitivity is 0."""
    exact = list(exact)
    res = evaluate(start, tau=TAU)
    f64_state = xm.f64().to_f64(evaluate(start, num=xm.f64())["state"]) if want else None
    moved = evaluate(nudged(start, seed, exact), **({"manifolds": res["manifolds"]} if nudge_on_res_manifolds else {}))
    res["sensitivity"] = scene_errors(scene, xm.native().to_f64(moved["state"]), res, start)
    if exact:
        res["sensitivity"][exact] = 0.0
    return res, f64_state


def momenta(num, before, after, state0):
    """Sum of m dx and of m x cross dx + I dtheta over the bodies, from the pose change of the Jacobi pass alone; dtheta is
    twice the vector part of dq q^-1."""
    lin, ang = 0, 0
    for k in range(len(state0)):
        m = 1.0 / state0[k, 0]
        inv = state0[k, 1:10].reshape(3, 3).T
        x0 = before[k, 31:34] + before[k, 28:31]
        dx = after[k, 31:34] - before[k, 31:34]
        dq = xm.qmul(after[k, 34:38][:, None], xm.conj(before[k, 34:38][:, None]))[:, 0]
        lin = lin + dx * m
        ang = ang + np.cross(x0, dx) * m + np.linalg.solve(inv, num.to_f64(dq[1:] * 2))
    return num.to_f64(lin), num.to_f64(ang)
