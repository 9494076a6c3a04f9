"""The yardstick of the mass-edit tests checked before it is used (tests/mass_edit_model.py), without a device.

DIRECT.  The model's inversion equals the committed oracle's o_mat3_invert and o_rigid_new (the transcription of Rigid::new) bit
for bit on 200 seeded random symmetric positive-definite tensors, and agrees with them that three crafted tensors are singular.

KEEP_FRAME.  The two formulas are held to their evaluation in exact rational arithmetic (fractions).  BOUND, worst case, with
u = 2^-53, Euclidean norms and a unit rotation (|qv x v| <= |v|, |s| <= 1), writing e(x) for the error of x:  c1 = qv x d has
|c1| <= |d| and e <= 3u|d| (two products and a difference per component);  t = c1 + d * s has |t| <= 2|d| and
e <= 3u|d| + u|d| + 2u|d| = 6u|d|;  c2 = qv x t has |c2| <= 2|d| and e <= 2 * 6u|d| + 3u * 2|d| = 18u|d|;  r = c2 * 2 + d has
|r| <= 5|d| and e <= 36u|d| + 5u|d| = 41u|d|.  Then position' = position + (r - d):  e <= 41u|d| + 6u|d| + u(|position| + 6|d|)
= u|position| + 53u|d|, and velocity' = velocity + w x r:  e <= 2|w| * 41u|d| + 3u|w| * 5|d| + u(|velocity| + 5|w||d|)
<= u|velocity| + 102u|w||d|.  Both are within 17 * u * S with S = |position| + 6|d| and S = |velocity| + 6|w||d|; the test asserts
that with |.| taken as sqrt(3) times the max norm (never smaller than the Euclidean norm) and prints the largest ratio it saw.
And the identity the flag is named after, frame' == frame, holds EXACTLY in rational arithmetic for any rotation, unit or not:
the operator is linear in the vector it turns."""
import math
from fractions import Fraction

import numpy as np

import mass_edit_model as mm
import oracle_binding as ob

U = 2.0 ** -53


def spd_tensors(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3)
        out.append(a @ a.T + np.eye(3) * 1e-3 * np.trace(a @ a.T))
    return out


def oracle_mat3(columns):
    return ob.Mat3(ob.vec3(columns[0]), ob.vec3(columns[1]), ob.vec3(columns[2]))


def test_direct_equals_the_oracles_invert_and_rigid_new_bit_for_bit():
    L = ob.load()
    rng = np.random.default_rng(77)
    for t in spd_tensors(200, 5000):
        cols = [tuple(float(v) for v in t[:, c]) for c in range(3)]          # column-major
        mass, com = float(10.0 ** rng.uniform(-3, 4)), rng.normal(size=3)
        verdict, out = mm.resolve([mass] + [v for c in cols for v in c] + list(com), mm.DIRECT)
        assert verdict == mm.OK
        inv = ob.Mat3()
        assert L.o_mat3_invert(oracle_mat3(cols), inv) == 1
        assert np.array(out[1:10]).tobytes() == inv.np().reshape(-1).tobytes()
        metrics = ob.Metrics(mass, 1.0, ob.vec3(com), oracle_mat3(cols))
        rigid = ob.Rigid()
        assert L.o_rigid_new(metrics, rigid) == 1
        r = rigid.np()
        assert np.array(out).tobytes() == r[mm.MASS_COLUMNS].tobytes()


def test_singular_tensors_are_singular_for_the_model_and_the_oracle():
    L = ob.load()
    crafted = {
        "a zero row": [(2.0, 0.0, 1.0), (0.5, 0.0, 3.0), (1.0, 0.0, 4.0)],       # row 1 of every column is zero
        "two equal columns": [(1.0, 2.0, 3.0), (1.0, 2.0, 3.0), (0.0, 1.0, 5.0)],
        "all zeros": [(0.0, 0.0, 0.0)] * 3,
    }
    for name, cols in crafted.items():
        verdict, out = mm.resolve([1.0] + [v for c in cols for v in c] + [0.0, 0.0, 0.0], mm.DIRECT)
        assert verdict == mm.SINGULAR and out is None, name
        assert L.o_mat3_invert(oracle_mat3(cols), ob.Mat3()) == 0, name
        rigid = ob.Rigid()
        assert L.o_rigid_new(ob.Metrics(1.0, 1.0, ob.vec3((0, 0, 0)), oracle_mat3(cols)), rigid) == 0, name


def test_the_value_rules_in_the_headers_order():
    good = [0.5] + [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] + [0.1, 0.2, 0.3]
    assert mm.resolve(good, mm.INVERSE) == (mm.OK, good)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for c in range(13):
            row = list(good)
            row[c] = bad
            assert mm.resolve(row, mm.INVERSE)[0] == mm.NOT_FINITE and mm.resolve(row, mm.DIRECT)[0] == mm.NOT_FINITE
    assert mm.resolve([-1e-300] + good[1:], mm.INVERSE)[0] == mm.NEGATIVE_INVERSE_MASS
    assert mm.resolve([-0.0] + good[1:], mm.INVERSE)[0] == mm.OK                 # -0.0 is not < 0
    assert mm.resolve([0.0] * 13, mm.INVERSE) == (mm.OK, [0.0] * 13) and mm.is_fixed([0.0] * 13)
    assert mm.resolve([0.0] + good[1:], mm.DIRECT)[0] == mm.MASS_NOT_POSITIVE
    assert mm.resolve([-2.0] + good[1:], mm.DIRECT)[0] == mm.MASS_NOT_POSITIVE
    verdict, out = mm.resolve([4.0] + good[1:], mm.DIRECT)
    assert verdict == mm.OK and out == [0.25] + good[1:]
    assert not mm.is_fixed(out)                                               # a DIRECT row always gives mass


def random_pose(rng, reach):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return (tuple(float(v) for v in rng.uniform(-reach, reach, 3)), tuple(float(v) for v in q), tuple(float(v) for v in rng.normal(size=3)),
            tuple(float(v) for v in rng.normal(scale=3.0, size=3)), tuple(float(v) for v in rng.uniform(-0.5, 0.5, 3)),
            tuple(float(v) for v in rng.uniform(-0.5, 0.5, 3)))


def exact(v):
    return tuple(Fraction(c) for c in v)


def test_keep_frame_is_within_the_derived_bound_of_its_exact_rational_evaluation():
    rng = np.random.default_rng(5100)
    worst = 0.0
    for k in range(300):
        pos, rot, vel, ang, com, com_new = random_pose(rng, 1e3 if k % 2 else 1.0)
        p, v = mm.keep_frame(pos, rot, vel, ang, com, com_new)
        pe, ve = mm.keep_frame(exact(pos), exact(rot), exact(vel), exact(ang), exact(com), exact(com_new))
        root3 = math.sqrt(3.0)
        d = root3 * max(abs(a - b) for a, b in zip(com_new, com))
        s_pos = root3 * max(abs(c) for c in pos) + 6.0 * d
        s_vel = root3 * max(abs(c) for c in vel) + 6.0 * root3 * max(abs(c) for c in ang) * d
        for c in range(3):
            ep, ev = abs(float(Fraction(p[c]) - pe[c])), abs(float(Fraction(v[c]) - ve[c]))
            assert ep <= 17 * U * s_pos and ev <= 17 * U * s_vel, (k, c, ep / (U * s_pos), ev / (U * s_vel))
            worst = max(worst, ep / (U * s_pos), ev / (U * s_vel))
    print("largest error of a KEEP_FRAME component: %.2f u S (bound 17)" % worst)


def test_keep_frame_leaves_the_frame_where_it_was_exactly_in_rational_arithmetic():
    rng = np.random.default_rng(5200)
    for k in range(100):
        pos, rot, vel, ang, com, com_new = (exact(v) for v in random_pose(rng, 1e3))
        if k % 3 == 0:
            rot = tuple(c * 3 for c in rot)                                   # not unit: the identity does not need it
        p, v = mm.keep_frame(pos, rot, vel, ang, com, com_new)
        assert mm.frame_origin(p, rot, com_new) == mm.frame_origin(pos, rot, com)
        # the new centre of mass is the material point that was at com_new - com from the old one: its velocity is v + w x r
        r = mm.qrot(rot, mm.sub(com_new, com))
        assert v == mm.add(vel, mm.cross(ang, r))
        assert mm.add(p, com_new) == mm.add(mm.add(pos, com), r)              # ... and it is where that point was


def test_apply_skips_what_the_device_skips_and_mixes_nothing():
    bodies = np.arange(4 * 38, dtype=np.float64).reshape(4, 38) + 1.0
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    rows = np.tile(np.array([2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.5, 0.5]), (5, 1))
    rows[1, 4] = np.nan
    rows[2, 0] = -1.0
    rows[3] = 0.0
    after, verdicts = mm.apply(bodies, [0, 1, 2, 3, 9], rows, mm.INVERSE, kinematic={0, 3})
    assert verdicts == [mm.KINEMATIC_RULE, mm.NOT_FINITE, mm.NEGATIVE_INVERSE_MASS, mm.OK, mm.OUT_OF_RANGE]
    assert after[:3].tobytes() == bodies[:3].tobytes()
    assert not after[3, mm.MASS_COLUMNS].any() and after[3, 10:28].tobytes() == bodies[3, 10:28].tobytes() and after[3, 31:38].tobytes() == bodies[3, 31:38].tobytes()
    moved, _ = mm.apply(bodies, [2], rows[:1], mm.INVERSE | mm.KEEP_FRAME)
    assert moved[2, 31:34].tobytes() == bodies[2, 31:34].tobytes()            # identity rotation: r == d, position + 0
    assert moved[2, 22:25].tobytes() != bodies[2, 22:25].tobytes()            # it spins: the new centre moves differently
