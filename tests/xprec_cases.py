"""The edge-body runs shared by test_xprec_oracle.py (oracle vs model, CPU) and test_gpu_xprec.py (HIP vs oracle and model):
the step configurations, the oracle's trajectory of each, the model re-seeded from it at every frame, and the bound.

Bound.  Per body and frame, with S substeps, eps = 2^-53, scale = |x| + extent (|x| the larger |position| at the frame's
start and end, extent the vertices' and the centre of mass's distance from the position) and h = dt / S:
    |position error| <= K S eps scale        |rotation error| <= K S eps scale / extent
    |velocity error| <= K S eps scale / h    |angular velocity error| <= K S eps scale / (extent h)
(derive divides x - x_past by h, so velocities carry the positions' rounding over h; a rotation is driven by the arm
c0 - (position + com), a difference of world points, so its rounding is that of |x| over the extent).  `normalized_errors` returns the
largest of the four ratios error / (S eps scale [/ h]), which must stay below K.
"""
import functools

import numpy as np

import edge_rigids as er
import oracle_binding as ob
import xprec_model as xm

EPS = 2.0 ** -53
# Measured on the edge bodies below with the oracle against the longdouble model (tests/test_xprec_oracle.py), largest
# normalized error of a checked body-frame per configuration: 404 with 1 substep, 304 with 4, 26 with 20 and 6.7 with 200
# (all at 1/60 s), and 1115 at dt = 1/10 s with 20 substeps (a body of inverse mass 0); 99 % of body-frames stay below 27.
# The error does not grow like S: it is set by single substeps in which a contact's arm c0 - (position + com) and
# x - past * local cancel large world coordinates.  K is 8x the largest measured value.
K = 9000.0
# A ground decision is compared only where the model's margin min |z| exceeds TAU.  A vertex height carries the error of
# the pose, which for the heights (they do not involve the far x, y) is below K S eps (|z| + extent) = 9000 * 200 * 1.1e-16
# * 2 m = 4e-10 m in the worst configuration here; TAU = 1e-9 m is above that and far below any contact depth.
TAU = 1e-9
# A constraint whose |c1 - c0| is below COND_MIN (normalize of a vector that short carries the rounding of c1 - c0,
# eps |x|, as a relative error of its direction), or a derive whose |delta.s| is below FLIP_MIN (the sign decides the
# angular velocity's sign), takes its body-frame out of the pose check; so does a frame whose exact result moves by more
# than SENSITIVITY_MAX (in the units of the bound) when the start state moves by one ulp: rounding the input alone then
# moves any f64 implementation that far (measured: 12 of 5 808 body-frames, all at dt = 1/10 s).
COND_MIN = 1e-9
FLIP_MIN = 1e-9
SENSITIVITY_MAX = 10.0
# (dt, substeps, frames): substeps 1, 4, 20 and 200 at 1/60 s, one case at 1/10 s
CONFIGS = ((1.0 / 60.0, 1, 40), (1.0 / 60.0, 4, 15), (1.0 / 60.0, 20, 6), (1.0 / 60.0, 200, 2), (1.0 / 10.0, 20, 3))
PER_CATEGORY = 8


def edge_case(config):
    dt, substeps, _ = CONFIGS[config]
    return er.generate(100 + config, PER_CATEGORY, h=dt / substeps)


def normalized_errors(got, model_state, start, ext, dt, substeps):
    """Per body: max over pose fields of |got - model| / (S eps scale [/ h]); model_state in the model's scalars."""
    h = dt / substeps
    num = xm.native()
    d = np.abs(num.to_f64(num.conv(got) - model_state))
    x = np.maximum(np.linalg.norm(start[:, 31:34], axis=1), np.linalg.norm(np.asarray(got)[:, 31:34], axis=1))
    scale = x + ext
    turn = scale / ext
    unit = substeps * EPS
    return np.max(np.stack([d[:, 31:34].max(axis=1) / (unit * scale), d[:, 34:38].max(axis=1) / (unit * turn),
                            d[:, 22:25].max(axis=1) * h / (unit * scale), d[:, 25:28].max(axis=1) * h / (unit * turn)]), axis=0)


def nudged(state, seed):
    """The dynamic state (velocity, angular velocity, position, rotation) moved by one ulp each, up or down at random."""
    rng = np.random.default_rng(seed)
    out = np.array(state, copy=True)
    cols = np.r_[22:28, 31:38]
    up = rng.random((out.shape[0], len(cols))) < 0.5
    out[:, cols] = np.where(up, np.nextafter(out[:, cols], np.inf), np.nextafter(out[:, cols], -np.inf))
    return out


def excluded(res):
    """Body-frames left out of the pose check: an ambiguous ground decision, an ill-conditioned constraint, a near-zero
    delta.s in derive, a frame that a one-ulp change of its start state moves by more than SENSITIVITY_MAX, or the
    reference outside its domain."""
    return ((res["margin"] <= TAU).any(axis=0) | (res["cond"] < COND_MIN).any(axis=0)
            | (res["flip_margin"] < FLIP_MIN).any(axis=0) | (res["sensitivity"] > SENSITIVITY_MAX) | ~res["domain"])


@functools.lru_cache(maxsize=None)
def trajectory(config):
    """The oracle over the config's frames, and the model stepped from the oracle's state at the start of every frame.
    Returns dict: start (n, 38), frames [(oracle state, oracle masks, model result)], labels, sid, verts, off, ext."""
    dt, substeps, frames = CONFIGS[config]
    bodies, sid, verts, off, labels = edge_case(config)
    ext = xm.extent(verts, off, sid, bodies)
    state, out = bodies, []
    for _ in range(frames):
        want, masks = ob.step_bodies(state, sid, verts, off, dt, substeps, want_masks=True)
        res = xm.step(state, verts, off, sid, dt, substeps)
        moved = xm.step(nudged(state, len(out)), verts, off, sid, dt, substeps)
        res["sensitivity"] = normalized_errors(xm.native().to_f64(moved["state"]), res["state"], state, ext, dt, substeps)
        out.append((state, want, masks, res))
        state = want
    return {"start": bodies, "frames": out, "labels": labels, "sid": sid, "verts": verts, "off": off, "ext": ext}


def check_against_model(config, got_frames, sel=None):
    """got_frames[f]: (state after frame f, masks of its substeps or None) of an implementation under test, for the bodies
    `sel` (default all) of the config.  Asserts masks and the bound; returns (normalized errors, excluded) (frames, n)."""
    dt, substeps, _ = CONFIGS[config]
    t = trajectory(config)
    sel = np.arange(len(t["labels"])) if sel is None else np.asarray(sel)
    errs, excl = [], []
    for f, (start, _, _, res) in enumerate(t["frames"]):
        got, masks = got_frames[f]
        if masks is not None:
            decided = res["margin"][:, sel] > TAU
            assert np.array_equal(np.where(decided, masks, 0), np.where(decided, res["masks"][:, sel], 0)), \
                "config %d frame %d: a ground decision with margin > %g differs from the model" % (config, f, TAU)
        e = normalized_errors(got, res["state"][sel], start[sel], t["ext"][sel], dt, substeps)
        x = excluded(res)[sel]
        bad = np.nonzero(~x & ~(e <= K))[0]
        assert not len(bad), "config %d frame %d: bodies %s (%s) beyond K = %g: %s" % (
            config, f, sel[bad[:8]], t["labels"][sel[bad[:8]]], K, e[bad[:8]])
        errs.append(e)
        excl.append(x)
    return np.array(errs), np.array(excl)
