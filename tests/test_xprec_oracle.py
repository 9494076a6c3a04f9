"""The f64 oracle against an independent extended-precision model of the reference (tests/xprec_model.py), on edge bodies
the scenes never produce (tests/edge_rigids.py).  Bit-identity with the oracle pins the kernels' operation order; these
tests pin the oracle's meaning: forces and torques in the body frame, asymmetric inverse inertia (M against its
transpose in all three products), frozen contact frames, derive's sign flip, the compliance.

Bound and thresholds: see xprec_cases.py (K, TAU, COND_MIN, FLIP_MIN, SENSITIVITY_MAX and the measured maxima)."""
import numpy as np
import pytest

import edge_rigids as er
import oracle_binding as ob
import xprec_cases as xc
import xprec_model as xm
from golden_util import load, max_rel, unhex


def test_longdouble_model_equals_mpmath_model():
    """The fast path and the 50-digit path of the model agree on 66 bodies of every category, 2^11 times inside the
    oracle's bound (measured: 0.006 in its units, K / 2^11 = 4.4).  In relative terms the largest difference is 9e-13,
    a far body's velocity ((x - x_past) / h at |x| = 1.4e4 m); the poses stay near 1e-18."""
    dt, substeps = 1.0 / 60.0, 20
    bodies, sid, verts, off, labels = er.generate(7, 6, h=dt / substeps)
    fast, ref = xm.native(), xm.mp(50)
    a = xm.step(bodies, verts, off, sid, dt, substeps, num=fast)
    b = xm.step(bodies, verts, off, sid, dt, substeps, num=ref)
    assert np.array_equal(a["masks"], b["masks"]) and a["masks"].any() and set(labels[a["masks"].any(axis=0)]) == set(er.CATEGORIES)
    if fast.name.startswith("mpmath"):
        exact = a["state"]
    else:                                                       # longdouble -> mpf exactly: a 64-bit significand is two doubles
        hi = a["state"].astype(np.float64)
        lo = (a["state"] - hi.astype(np.longdouble)).astype(np.float64)
        exact = ref.conv(hi) + ref.conv(lo)
    # in the units of the oracle's bound (xprec_cases.normalized_errors with eps = 2^-53), the fast path must sit 2^11
    # times inside K: it is the yardstick the f64 oracle is held to
    diff = np.abs(ref.to_f64(exact - b["state"]))
    x = np.linalg.norm(bodies[:, 31:34], axis=1)
    ext = xm.extent(verts, off, sid, bodies)
    scale, turn, h, unit = x + ext, (x + ext) / ext, dt / substeps, substeps * xc.EPS
    e = np.max(np.stack([diff[:, 31:34].max(axis=1) / (unit * scale), diff[:, 34:38].max(axis=1) / (unit * turn),
                         diff[:, 22:25].max(axis=1) * h / (unit * scale), diff[:, 25:28].max(axis=1) * h / (unit * turn)]), axis=0)
    assert e.max() <= xc.K / 2 ** 11, e.max()
    assert (diff / np.maximum(np.abs(ref.to_f64(b["state"])), 1.0)).max() < 1e-12


@pytest.mark.parametrize("config", range(len(xc.CONFIGS)), ids=["dt%.4g-S%d" % c[:2] for c in xc.CONFIGS])
def test_oracle_against_the_model_frame_by_frame(config):
    """Every frame re-seeds the model from the oracle's f64 state (exactly) and steps both: every ground decision with a
    margin above TAU equals the model's, and every well-conditioned body-frame is within the bound."""
    t = xc.trajectory(config)
    errs, excl = xc.check_against_model(config, [(want, masks) for (_, want, masks, _) in t["frames"]])
    assert excl.mean() < 0.10, excl.mean()
    for cat in er.CATEGORIES:
        assert (~excl[:, t["labels"] == cat]).any(), cat                  # every category keeps checked cases


def test_exclusions_are_rare():
    """Under 5 % of all body-frames are left out of the pose check (measured: 12 of 5 808)."""
    n = excluded = 0
    for config in range(len(xc.CONFIGS)):
        for _, _, _, res in xc.trajectory(config)["frames"]:
            x = xc.excluded(res)
            n, excluded = n + x.size, excluded + int(x.sum())
    assert excluded < 0.05 * n, (excluded, n)


def test_every_category_makes_ground_contacts_and_asymmetric_bodies_spin_in_contact():
    contacts = {c: 0 for c in er.CATEGORIES}
    spinning_asym = 0
    for config in range(len(xc.CONFIGS)):
        t = xc.trajectory(config)
        for start, want, masks, _ in t["frames"]:
            for c in er.CATEGORIES:
                contacts[c] += int((masks[:, t["labels"] == c] != 0).sum())
            asym = t["labels"] == "asym_inertia"
            torque = np.abs(start[:, 16:22]).max(axis=1) > 0
            spin = np.linalg.norm(start[:, 25:28], axis=1) > 1.0
            m = start[:, 1:10].reshape(-1, 3, 3)
            skew = np.abs(m - m.transpose(0, 2, 1)).max(axis=(1, 2)) > 0.1 * np.abs(m).max(axis=(1, 2))
            # integrate's M * torque, inverse_resitance's M * a and apply_impulse's M * arm all live in one frame
            spinning_asym += int((asym & torque & spin & skew & (masks != 0).any(axis=0)).sum())
    assert all(v > 0 for v in contacts.values()), contacts
    assert spinning_asym >= 20, spinning_asym


def test_derive_sign_flip_is_reached():
    """derive's `delta.s < 0` branch (rigid.rs:104-106): within one substep some bodies turn by more than half a turn,
    mostly by the impulses of deep contacts in long substeps (measured: 103 substeps, 68 of them at S = 1, 14 at S = 4,
    21 at dt = 1/10).  The model counts them, and the frame-by-frame test holds the oracle to the model there."""
    flips = sum(int(res["flip"].sum()) for config in range(len(xc.CONFIGS)) for _, _, _, res in xc.trajectory(config)["frames"])
    assert flips >= 20, flips


def test_exact_heights_are_outside_the_model_only_where_the_square_is_not_normal(oracle):
    """The exact heights of edge_rigids.exact_heights(): z = +-0 makes no contact (`z >= 0`, collision.rs:18), every
    negative height does; the model leaves the reference's domain exactly where correction.correction = z^2 is not a
    normal f64, and the oracle turns NaN exactly where that square is 0."""
    bodies, sid, verts, off, labels = er.exact_heights()
    res = xm.step(bodies, verts, off, sid, 1.0 / 60.0, 1)
    want, masks = ob.step_bodies(bodies, sid, verts, off, 1.0 / 60.0, 1, want_masks=True)
    z = bodies[:, 33]
    assert np.array_equal(masks[0] != 0, z < 0) and np.array_equal(res["masks"][0] != 0, z < 0)
    assert np.array_equal(res["domain"], ~((z < 0) & (z * z < xm.F64_MIN_NORMAL)))
    with np.errstate(under="ignore"):
        assert np.array_equal(np.isnan(want).any(axis=1), (z < 0) & (z * z == 0.0))
    ok = res["domain"]
    got = np.asarray(xm.native().to_f64(res["state"]))
    assert np.abs(got[ok][:, 22:38] - want[ok][:, 22:38]).max() < 1e-12


@pytest.mark.parametrize("name", ["world_new", "config1_boxes32"])
def test_golden_scene_stays_within_the_north_star_of_the_model(name):
    """The golden scenes whose whole length lies inside the f64-vs-exact horizon (scripts/xprec_horizon.py: world_new
    first passes 1e-5 at frame 62 of 60, config1_boxes32 at frame 38 of 30): the model, run from the same start and
    never re-seeded, gives every substep's masks of the golden file and poses within 1e-5 relative of it."""
    d = load(name + ".json")
    verts, off = unhex(d["verts"], (-1, 3)), np.array(d["vert_offsets"], dtype=np.uint32)
    state = unhex(d["initial"], (-1, 38))
    sid = np.array(d.get("shape_id", [0] * len(state)), dtype=np.uint32)
    frames = len(d["masks"])
    for f in range(frames):
        res = xm.step(state, verts, off, sid, float.fromhex(d["dt"]), d["substeps"])
        state = res["state"]
        assert np.array_equal(res["masks"], np.array(d["masks"][f], dtype=np.uint32)), f
        if "frames" in d:
            assert max_rel(xm.native().to_f64(state)[:, 31:38], unhex(d["frames"][f], (-1, 38))[:, 31:38]) <= 1e-5, f
    assert max_rel(xm.native().to_f64(state)[:, 31:38], unhex(d["final"] if "final" in d else d["frames"][-1], (-1, 38))[:, 31:38]) <= 1e-5
