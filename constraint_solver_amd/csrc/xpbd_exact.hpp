// xpbd_exact.hpp -- two correctly rounded f64 primitives for the shapes in which the stepper uses `/` and `sqrt` (it uses
// the first; the second was measured and is not: see "div_by" below):
//
//   sqrt_and_reciprocal(a, s, k)      s = RN(sqrt(a)), k = RN(1 / s)     from ONE reciprocal-square-root seed
//   div_by(x, h, inv_h, h_ok)         RN(x / h)                          for a divisor known before the launch
//
// Both return, bit for bit, what `sqrt(a)`, `1.0 / sqrt(a)` and `x / h` return; only the instruction sequence differs
// from the compiler's general expansions (which scale every operand into range and, for `1.0 / s`, start again from a
// reciprocal seed although the square-root iteration already carries 1/(2 sqrt(a))).  Every fused multiply-add is an
// explicit __builtin_fma: the translation units stay at -ffp-contract=off.
//
// Each primitive has a fast path, valid inside a window of exponents in which no intermediate overflows, underflows or
// loses bits, and the plain expression for every other operand (zero where it matters, subnormals, huge values,
// infinities, NaN).  The windows are far narrower than the sequences need; they are chosen so that the argument is short.
//
// Host builds: with XPBD_EXACT_RSQ_SEED(a) defined before this header is included (tests/exact_math_host.cpp injects a
// perturbed seed) the same sequences compile for the host; in the host pass of a HIP unit the pair is the plain one.
#pragma once

#include <cstdint>
#include <cstring>

#include "xpbd_math.hpp"

#if !defined(XPBD_EXACT_RSQ_SEED) && defined(__HIP_DEVICE_COMPILE__)
#define XPBD_EXACT_RSQ_SEED(a) __builtin_amdgcn_rsq(a) // v_rsq_f64
#endif

namespace xpbd {
namespace exact {

XPBD_HD uint64_t bits_of(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}
XPBD_HD double from_bits(uint64_t u)
{
    double v;
    memcpy(&v, &u, sizeof v);
    return v;
}
XPBD_HD uint32_t high_word(double v) { return (uint32_t)(bits_of(v) >> 32); }

// ---- sqrt_and_reciprocal -------------------------------------------------------------------------------------------
// Window of a: 2^-500 <= a < 2^501, tested on the high dword (sign, exponent); a negative a, a NaN, an infinity, a zero
// and a subnormal all fail the one unsigned compare.
constexpr uint32_t kPairExpLo = (1023u - 500u) << 20, kPairExpSpan = 1001u << 20;
XPBD_HD bool pair_in_window(double a) { return high_word(a) - kPairExpLo < kPairExpSpan; }

#if defined(XPBD_EXACT_RSQ_SEED)
// The fast path.  y0 is a seed for 1/sqrt(a) of relative error delta (v_rsq_f64: well below 2^-20).
//
// Square root: the chain below IS the backend's expansion of sqrt(double) for gfx950 (one coupled Newton step on
// g ~ sqrt(a), hh ~ 1/(2 sqrt(a)), then two residual steps g += (a - g*g) * hh), without its range scaling: the backend
// multiplies a by 2^256 only when a < 2^-767 and handles 0 and +inf by a select.  For a in the window neither happens,
// so s is the backend's sqrt(a) by construction -- the same operations on the same values.
//
// Reciprocal: after the coupled step hh = (1 / (2 sqrt(a))) (1 + e0) with |e0| <= 1.5 delta^2 + 2^-51 < 2^-38, and
// s = sqrt(a) (1 + e_s) with |e_s| <= 2^-53.  y = hh + hh is exact.  One Newton step y' = y + (1 - s y) y squares the
// error of y against 1/s (< 2^-37) and adds two roundings, so y' is within 1/2 ulp + 2^-70 of 1/s: within one ulp.
// Markstein's theorem (P. Markstein 1990; Muller et al., Handbook of Floating-Point Arithmetic, "Division with an FMA")
// then says of the second step: if y' is within one ulp of 1/s, e = fma(-s, y', 1) is exact and fma(e, y', y') =
// RN(1/s), PROVIDED the significand of s is not all ones.  That exception is real and sits where unit quaternions live
// (a = 1 - 2^-53 gives s = 2 - 2^-52 scaled): there 1/s = 2^-e-1 (1 + 2^-53 + ...) lies just above a midpoint, the step
// returns 2^-e-1 or its successor depending on y', and RN(1/s) is the successor 2^-e-1 (1 + 2^-52).  Both candidates
// have the same high dword and the right one has low dword 1, so an all-ones s sets k's low dword to 1 (four integer
// instructions, no branch).
//
// The window: with 2^-500 <= a < 2^501, every value of the chain lies between 2^-610 and 2^501 in magnitude or is an
// exact zero residual (g, s in [2^-250, 2^251); hh, y, k in (2^-252, 2^251); the residuals a - g*g are at least
// a 2^-106 when not zero; r and e are absolute quantities of at least 2^-107 when not zero), so nothing overflows,
// underflows or is rounded in the subnormal range.
XPBD_HD void sqrt_and_reciprocal_fast(double a, double &s, double &k)
{
    const double y0 = XPBD_EXACT_RSQ_SEED(a);
    double g = a * y0;
    double hh = y0 * 0.5;
    const double r = __builtin_fma(-hh, g, 0.5);
    g = __builtin_fma(g, r, g);
    hh = __builtin_fma(hh, r, hh);
    double d = __builtin_fma(-g, g, a);
    g = __builtin_fma(d, hh, g);
    d = __builtin_fma(-g, g, a);
    g = __builtin_fma(d, hh, g);
    double y = hh + hh;
    double e = __builtin_fma(-g, y, 1.0);
    y = __builtin_fma(e, y, y);
    e = __builtin_fma(-g, y, 1.0);
    y = __builtin_fma(e, y, y);
    const uint64_t sb = bits_of(g), yb = bits_of(y);
    const uint32_t ones = ((uint32_t)(sb >> 32) | 0xfff00000u) & (uint32_t)sb; // 0xffffffff <=> significand all ones
    s = g;
    k = from_bits((yb & 0xffffffff00000000ull) | (ones == 0xffffffffu ? 1u : (uint32_t)yb));
}

// s = RN(sqrt(a)), k = RN(1 / s) for every a: lanes outside the window take the plain expressions, out of line.
XPBD_HD void sqrt_and_reciprocal(double a, double &s, double &k)
{
    sqrt_and_reciprocal_fast(a, s, k);
    if (__builtin_expect(!pair_in_window(a), 0)) {
        s = sqrt(a);
        k = 1.0 / s;
    }
}
#else
XPBD_HD void sqrt_and_reciprocal(double a, double &s, double &k)
{
    s = sqrt(a);
    k = 1.0 / s;
}
#endif

// ---- div_by --------------------------------------------------------------------------------------------------------
// NOT used by the stepper: derive_body's six quotients by h keep the plain `/`.  With the guard below the sequence is no
// shorter than the compiler's expansion in k_step (120 against 114 VALU instructions in derive), and in the A/B it was
// inside the spread alone and a loss on top of the pair ("Correctly rounded 1/sqrt from one seed").  It
// stays as a checked building block: xpbd_selftest_exact_math and the host check evaluate it next to the pair.
//
// The divisor's side, once per launch: h positive and normal with 2^-64 <= h < 2^64, and its significand not all ones
// (no step below needs the last condition; it keeps h away from the one divisor for which a reciprocal iteration is
// known to misround, at no cost).  inv_h = 1.0 / h is formed next to it, by the correctly rounded division.
XPBD_HD bool divisor_ok(double h)
{
    const uint64_t b = bits_of(h);
    const uint32_t hi = (uint32_t)(b >> 32);
    return hi - ((1023u - 64u) << 20) < (128u << 20) && (b & 0x000fffffffffffffull) != 0x000fffffffffffffull;
}

// What a launcher hands its kernel next to the divisor (wave-uniform: it sits in scalar registers).
struct Divisor {
    double h, inv_h;
    uint32_t ok;
};
XPBD_HD Divisor divisor(double h) { return Divisor{h, 1.0 / h, divisor_ok(h) ? 1u : 0u}; }

// Window of x: an exact zero of either sign, or 2^-400 <= |x| < 2^401.
constexpr uint32_t kDivExpLo = (1023u - 400u) << 20, kDivExpSpan = 801u << 20;
XPBD_HD bool dividend_in_window(double x)
{
    const uint64_t b = bits_of(x);
    const uint32_t t = (uint32_t)(b >> 32) & 0x7fffffffu;
    return (t | (uint32_t)b) == 0u || t - kDivExpLo < kDivExpSpan;
}

// The fast path: RN(x / h) from r = RN(1 / h) in one multiply and four fma.  Write t = x / h and u = ulp(t).
//   q1 = RN(x r):       r = (1/h)(1 + e_r) with |e_r| <= 2^-53, so |q1 - t| < 3/2 u (one ulp from r, half from the rounding).
//   e1 = RN(x - q1 h):  h (t - q1) to one rounding (it is exact when |q1 - t| <= u, not always beyond).
//   q2 = RN(q1 + e1 r): q1 + e1 r = t + (q1 - t) O(2^-51), so |q2 - t| <= u/2 + 2^-50 u: within one ulp.
//   e2 = x - q2 h, q3 = RN(q2 + e2 r):  Markstein's theorem for the quotient (Markstein 1990; Handbook of Floating-Point
//       Arithmetic, "Division with an FMA"): if r = RN(1/h) and q2 is within one ulp of x/h, then e2 is exact and
//       q3 = RN(x / h).  There is no exceptional divisor in this statement.
// The three-operation form (q1, e1, q2 alone; Brisebarre, Muller and Raina 2004 analyse it for a divisor known in
// advance) is NOT used: q1 can be more than one ulp off, the theorem's condition, and for which divisors the shorter
// form still rounds every x correctly has to be checked divisor by divisor.
// Signs: h > 0, so the quotient has x's sign; for x = -0 the sequence gives +0, so the sign bit is copied from x.
// The window: |x| in [2^-400, 2^401) and h in [2^-64, 2^64) keep q in [2^-465, 2^466) and the residuals, which are at
// least 2^-107 |x| when not zero, above 2^-507: nothing overflows, underflows or is rounded in the subnormal range.
XPBD_HD double div_by_fast(double x, double h, double inv_h)
{
    double q = x * inv_h;
    double e = __builtin_fma(-q, h, x);
    q = __builtin_fma(e, inv_h, q);
    e = __builtin_fma(-q, h, x);
    q = __builtin_fma(e, inv_h, q);
    return __builtin_copysign(q, x);
}

// RN(x / h) for every x and h, with h_ok = divisor_ok(h) and inv_h = 1.0 / h: operands outside the windows take the plain
// quotient, out of line.
XPBD_HD double div_by(double x, double h, double inv_h, bool h_ok)
{
    double q = div_by_fast(x, h, inv_h);
    if (__builtin_expect(!(h_ok && dividend_in_window(x)), 0))
        q = x / h;
    return q;
}

// One guard for the three components.
XPBD_HD Vec3 div_by(Vec3 v, double h, double inv_h, bool h_ok)
{
    Vec3 q{div_by_fast(v.x, h, inv_h), div_by_fast(v.y, h, inv_h), div_by_fast(v.z, h, inv_h)};
    if (__builtin_expect(!(h_ok && dividend_in_window(v.x) && dividend_in_window(v.y) && dividend_in_window(v.z)), 0))
        q = v / h;
    return q;
}

XPBD_HD Vec3 div_by(Vec3 v, const Divisor &d) { return div_by(v, d.h, d.inv_h, d.ok != 0u); }

} // namespace exact
} // namespace xpbd
