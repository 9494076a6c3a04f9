"""The stepper's two short sequences (constraint_solver_amd/csrc/xpbd_exact.hpp) on the device.

1. xpbd_selftest_exact_math on about 4e6 operands of the families of tests/exact_math_host.cpp, plus subnormals, +-inf
   and NaN: the device's fast results equal the device's plain results, the plain results equal NumPy's `x / h`,
   `np.sqrt(a)` and `1.0 / np.sqrt(a)`, all bit for bit (NaN-ness for NaN), and the two all-ones cases are pinned by value.
2. The stepper against the oracle on 65 and 130 bodies (one full wave and a partial one; two and a partial one): boxes in
   resting contact with hand-set lanes in the same waves that take the slow paths or sit on the sequences' special
   values.  All 38 doubles and every substep's mask bit-identical, fused and per substep."""
import numpy as np
import pytest

import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
ALL_ONES = (1 << 52) - 1


def make(sig, exp, neg=False):
    """The double with 52-bit significand field `sig` and unbiased exponent `exp`."""
    sig = np.asarray(sig, dtype=np.uint64) & np.uint64(ALL_ONES)
    bits = (np.asarray(exp, dtype=np.int64) + 1023).astype(np.uint64) << np.uint64(52) | sig
    bits = bits | (np.asarray(neg, dtype=np.uint64) << np.uint64(63))
    return bits.view(np.float64)


def neighbours(values, k):
    """Every value with its k predecessors and k successors (in bit order; finite values only make sense)."""
    bits = np.asarray(values, dtype=np.float64).view(np.int64)
    return (bits[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).reshape(-1).view(np.float64)


def pair_operands(rng):
    one = np.float64(1.0).view(np.int64)
    near_one = (one + np.arange(-(1 << 24), (1 << 24) + 1, 16, dtype=np.int64)).view(np.float64)  # every 16th double within 2^24 ulp
    nearest = (one + np.arange(-8192, 8193, dtype=np.int64)).view(np.float64)                     # ... and all of the nearest
    exps = np.repeat(np.arange(-503, 504), 4)
    patterns = make(np.tile(np.array([ALL_ONES, ALL_ONES - 1, 0, 1], dtype=np.uint64), 1007), exps)
    r = rng.integers(1, 1 << 26, 150000).astype(np.float64)
    squares = np.ldexp(r * r, 2 * rng.integers(-245, 245, r.size))
    squares = np.concatenate([squares, np.nextafter(squares, 0.0), np.nextafter(squares, np.inf)])
    random = make(rng.integers(0, 1 << 52, 1200000, dtype=np.uint64), rng.integers(-500, 501, 1200000))
    s = make(np.full(100000, ALL_ONES, dtype=np.uint64), rng.integers(-250, 250, 100000))   # roots with an all-ones significand
    sq = s * s
    ones_roots = np.concatenate([sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)])
    edges = neighbours([2.0 ** -500, 2.0 ** 501, 2.0 ** -767, 2.0 ** -1022, 1.0, 4.0], 64)
    special = np.array([0.0, -0.0, 5e-324, 2.0 ** -1060, 2.0 ** -1023, np.finfo(np.float64).max, np.inf, -np.inf, np.nan, -1.0, -2.0 ** -600,
                        1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52])
    subnormal = rng.integers(1, 1 << 52, 2000, dtype=np.uint64).view(np.float64)
    return np.concatenate([near_one, nearest, patterns, squares, random, ones_roots, edges, special, subnormal])


def divisors():
    hs = [(1.0 / 60.0) / k for k in range(1, 40)]
    hs += [1.0 / 60.0, 0.001, 1.0 / 3.0, 1.0 / 30.0, 1.0 / 120.0, 0.01, 1.0]
    hs += [float(make(ALL_ONES, -7)), float(make(ALL_ONES - 1, -7))]      # all-ones significand: the divisor's guard says no
    hs += [2.0 ** -64, float(np.nextafter(2.0 ** -64, 0.0)), float(np.nextafter(2.0 ** 64, 0.0)), 2.0 ** 64]   # the guard's edges
    return hs


def hard_quotients(h):
    """x with x / h within |c| 2^-106 (relative) of the midpoint of two doubles, built from h with integer arithmetic:
    H = odd part of h's significand (b bits), N an odd 54-bit integer with N H = c (mod 2^m), X = (N H - c) / 2^m."""
    H = (int(np.float64(h).view(np.uint64)) & ALL_ONES) | (1 << 52)
    while H % 2 == 0:
        H >>= 1
    b = H.bit_length()
    out = []
    if b < 40:
        return out
    for m in (b, b + 1):
        if m > 54:
            continue
        inv = pow(H, -1, 1 << m)
        for c in range(-255, 256, 2):
            N = (c * inv) % (1 << m)
            while N < (1 << 54):
                if N >= (1 << 53):
                    X, rem = divmod(N * H - c, 1 << m)
                    if rem == 0 and (1 << 52) <= X < (1 << 53):
                        out.append(float(X))
                N += 1 << m
    return out


def dividends(rng, h, n):
    random = make(rng.integers(0, 1 << 52, n, dtype=np.uint64), rng.integers(-400, 401, n), rng.integers(0, 2, n))
    edges = neighbours([2.0 ** -400, -2.0 ** -400, 2.0 ** 401, -2.0 ** 401, 2.0 ** -1022], 16)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1043, 2.0 ** -1060, np.finfo(np.float64).max, np.inf, -np.inf, np.nan])
    hard = np.array(hard_quotients(h), dtype=np.float64)
    hard = np.concatenate([np.ldexp(hard, rng.integers(-400, 300, hard.size)), -np.ldexp(hard, -52)])
    return np.concatenate([hard, edges, special, random])[:n]


def same_or_both_nan(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bits_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want))


def test_device_sequences_agree_with_the_plain_expressions_and_with_numpy():
    rng = np.random.default_rng(11)
    a_all = pair_operands(rng)
    assert 3.5e6 < a_all.size < 4.5e6
    hs = divisors()
    chunks = np.array_split(a_all, len(hs))
    for h, a in zip(hs, chunks):
        x = dividends(rng, h, a.size)
        assert x.size == a.size
        fast, plain = capi.selftest_exact_math(x, a, h)
        with np.errstate(all="ignore"):
            root = np.sqrt(a)
            want = np.stack([x / h, root, 1.0 / root])
        for row, what in enumerate(["x / h", "sqrt(a)", "1 / sqrt(a)"]):
            assert same_or_both_nan(plain[row], want[row]), (what, "device plain against NumPy", h)
            assert same_or_both_nan(fast[row], plain[row]), (what, "device fast against device plain", h)


def test_device_reciprocal_of_an_all_ones_root_is_pinned_by_value():
    a = np.array([1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 1.0, 4.0 * (1.0 - 2.0 ** -53)])
    fast, plain = capi.selftest_exact_math(np.zeros(a.size), a, DT)
    for got in (fast, plain):
        assert got[1].tolist() == [1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53, 1.0, 2.0 - 2.0 ** -52]      # 0x1.fffffffffffffp-1, ...p+0
        assert got[2].tolist() == [1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, 1.0, 0.5 * (1.0 + 2.0 ** -52)]


# ---------------------------------------------------------------- the stepper, fast and slow lanes in one wave
VEL, ANG, POS, ROT = slice(22, 25), slice(25, 28), slice(31, 34), slice(34, 38)
FORCES = slice(10, 22)   # external / internal force, external / internal torque


def squared_norm(q):
    """normalized(Quat)'s m2, in its order: s*s + ((x*x + y*y) + z*z), IEEE double operation by operation."""
    s, x, y, z = (np.float64(v) for v in q)
    return s * s + (x * x + y * y + z * z)


def hand_set(bodies, base):
    """Six special bodies from lane `base` on, every seventh lane: none has a force or torque, so its first integration
    leaves the rotation's components as set."""
    lanes = [base + 7 * k for k in range(6)]
    for i in lanes:
        bodies[i, FORCES] = 0.0
        bodies[i, VEL] = 0.0
        bodies[i, ANG] = 0.0
        bodies[i, POS] = [0.5 * i, 0.25, 5.0]                   # above the ground
        bodies[i, ROT] = [1.0, 0.0, 0.0, 0.0]                   # exactly unit: m2 = 1.0
    still, huge, tiny, unit, below_a, below_b = lanes
    # `still` does not move at all: every delta of derive is an exact zero of one sign or the other
    bodies[huge, POS] = [1e300, -1e300, 1e300]                  # quotients far above the window
    bodies[huge, VEL] = [1e290, 1e290, 0.0]
    bodies[tiny, POS] = [0.0, 0.0, 5.0]
    bodies[tiny, VEL] = [1e-300, -1e-300, 0.0]                  # deltas far below the window
    # squared norms whose root has an all-ones significand: 1 - 2^-53 and 1 - 2^-52
    bodies[below_a, ROT] = [1.0 - 2.0 ** -53, 2.0 ** -26.5, 0.0, 0.0]
    bodies[below_b, ROT] = [1.0 - 2.0 ** -53, 0.0, 0.0, 0.0]
    assert squared_norm(bodies[unit, ROT]) == 1.0
    assert squared_norm(bodies[below_a, ROT]) == 1.0 - 2.0 ** -53
    assert squared_norm(bodies[below_b, ROT]) == 1.0 - 2.0 ** -52
    return lanes


@pytest.fixture(scope="module")
def stepper_cases():
    """n -> (bodies, shape ids, vertices, offsets, oracle states per frame, oracle masks per frame); computed once."""
    verts, off = capi.scene_shapes(capi.SCENE_BOXES)
    cases = {}
    for n in (65, 130):
        bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 5, n)
        # at rest on the ground: the unit cubes' lower faces a micrometre inside it, a random yaw, a micro-radian of tilt
        rng = np.random.default_rng(3)
        yaw, tilt = rng.uniform(0.0, np.pi, n), rng.normal(0.0, 1e-6, (n, 2))
        q = np.stack([np.cos(yaw / 2), tilt[:, 0], tilt[:, 1], np.sin(yaw / 2)], axis=1)
        bodies[:, ROT] = q / np.linalg.norm(q, axis=1, keepdims=True)
        bodies[:, 33] = -1e-6
        bodies[:, VEL] = 0.0
        bodies[:, ANG] = 0.0
        special = hand_set(bodies, 2)
        if n > 64:
            special += [64] if n == 65 else hand_set(bodies, 66)
        if n == 65:                                              # the partial wave's only lane is a special one
            bodies[64, ROT] = [1.0 - 2.0 ** -53, 0.0, 0.0, 0.0]
        want, states, masks = bodies, [], []
        for _ in range(3):
            want, m = ob.step_bodies(want, sid, verts, off, DT, 20, want_masks=True, threads=8)
            states.append(want)
            masks.append(m)
        cases[n] = (bodies, sid, verts, off, states, masks, special)
    return cases


@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
@pytest.mark.parametrize("n", [65, 130])
def test_stepper_with_fast_and_slow_lanes_in_one_wave_matches_the_oracle(stepper_cases, n, mode):
    bodies, sid, verts, off, states, masks, special = stepper_cases[n]
    with capi.World(mode=mode, trace_contacts=True) as w:
        w.set_shapes(verts, off)
        w.upload(bodies, sid)
        for frame in range(3):
            w.step(DT, 20)
            assert np.array_equal(w.contact_masks(20), masks[frame]), frame   # every substep's mask
            got = w.download()
            assert not np.isnan(states[frame]).any()
            assert bits_equal(got, states[frame]), frame                      # all 38 doubles
    resting = np.setdiff1d(np.arange(n), special)
    assert (np.array(masks)[:, :, resting] != 0).all()                        # the boxes are in ground contact in every substep
    assert not np.array(masks)[:, :, special[:6]].any()                       # ... and the hand-set lanes are not
