// exact_math_host.cpp -- host check of constraint_solver_amd/csrc/xpbd_exact.hpp (built and run by
// tests/test_exact_math_host.py with g++ -O2 -ffp-contract=off).  The reciprocal-square-root seed is injected as
// (1 / sqrt(a)) (1 + delta) with |delta| <= 2^-20 (no error bound for v_rsq_f64 is documented where this was written, so
// the fall-back figure is used: far coarser than the instruction).  Every result is compared bit for bit with `/` and
// `sqrt`; the program prints the operand counts and exits 0 only with zero differences.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

static double g_delta = 0.0;
#define XPBD_EXACT_RSQ_SEED(a) ((1.0 / sqrt(a)) * (1.0 + g_delta))
#include "xpbd_exact.hpp"

using namespace xpbd::exact;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() // xorshift64*
{
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}
static double make(uint64_t significand52, int exponent, bool negative = false)
{
    return from_bits(((uint64_t)negative << 63) | ((uint64_t)(exponent + 1023) << 52) | (significand52 & 0x000fffffffffffffull));
}
static bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

static unsigned long long n_pair = 0, n_pair_fast = 0, bad_root = 0, bad_recip = 0;
static unsigned long long n_div = 0, n_div_fast = 0, bad_div = 0;

static const double kDeltas[] = {0.0, 0x1p-20, -0x1p-20, 0x1p-21, -0x1.8p-21, 0x1p-30, -0x1p-26};
static void next_delta()
{
    const uint64_t r = rnd();
    g_delta = (r & 8) ? kDeltas[r % 7] : ((double)(int64_t)(r >> 11) * 0x1p-52 - 1.0) * 0x1p-20;
}

static void check_pair(double a)
{
    double s, k;
    next_delta();
    sqrt_and_reciprocal(a, s, k);
    const double ws = sqrt(a), wk = 1.0 / ws;
    ++n_pair;
    n_pair_fast += pair_in_window(a);
    if (!same(s, ws) && bad_root++ < 10)
        printf("root: a=%a delta=%a got %a want %a\n", a, g_delta, s, ws);
    if (!same(k, wk) && bad_recip++ < 10)
        printf("recip: a=%a delta=%a got %a want %a\n", a, g_delta, k, wk);
}

static void check_div(double x, double h)
{
    const double inv_h = 1.0 / h;
    const bool h_ok = divisor_ok(h);
    const double q = div_by(x, h, inv_h, h_ok), w = x / h;
    ++n_div;
    n_div_fast += h_ok && dividend_in_window(x);
    if (!same(q, w) && bad_div++ < 10)
        printf("div: x=%a h=%a got %a want %a\n", x, h, q, w);
    // the Vec3 form shares one guard: x next to a fast and next to a slow neighbour
    const xpbd::Vec3 v = div_by(xpbd::Vec3{x, 1.0, -0.0}, h, inv_h, h_ok), u = div_by(xpbd::Vec3{0x1p-1000, x, 3.0}, h, inv_h, h_ok);
    if (!(same(v.x, w) && same(v.y, 1.0 / h) && same(v.z, -0.0 / h) && same(u.x, 0x1p-1000 / h) && same(u.y, w) && same(u.z, 3.0 / h)) && bad_div++ < 10)
        printf("div (Vec3): x=%a h=%a\n", x, h);
}

// x whose quotient x / h lies within |c| 2^-106 (relative) of the midpoint of two neighbouring doubles: with H the odd part
// of h's significand (b bits) and N an odd 54-bit integer (a midpoint), X = (N H - c) / 2^m is an integer for
// N = c / H (mod 2^m), and X / H = (N - c / H) / 2^m.  m = b or b + 1 puts X in [2^52, 2^53).
static void hard_quotients(double h)
{
    uint64_t H = (bits_of(h) & 0x000fffffffffffffull) | (1ull << 52);
    while (!(H & 1))
        H >>= 1;
    const int b = 64 - __builtin_clzll(H);
    if (b < 40) // a short divisor (a power of two, say) has no quotient that close to a midpoint
        return;
    uint64_t inv = H; // Newton: inverse of H modulo 2^64
    for (int i = 0; i < 6; ++i)
        inv *= 2 - H * inv;
    for (int m = b; m <= b + 1 && m <= 54; ++m) {
        const uint64_t mask = m == 64 ? ~0ull : (1ull << m) - 1;
        for (int64_t c = -2047; c <= 2047; c += 2) {
            const uint64_t n0 = ((uint64_t)c * inv) & mask;
            for (uint64_t N = n0; N < (1ull << 54); N += mask + 1) {
                if (N < (1ull << 53))
                    continue;
                const unsigned __int128 p = (unsigned __int128)N * H - (__int128)c;
                const uint64_t X = (uint64_t)(p >> m);
                if ((p & mask) != 0 || X < (1ull << 52) || X >= (1ull << 53))
                    continue;
                const int e = (int)(rnd() % 700) - 350;
                check_div(ldexp((double)X, e - 52), h);
                check_div(-ldexp((double)X, -52), h);
            }
        }
    }
}

int main()
{
    // ---- the pair ----
    const uint64_t one = bits_of(1.0);
    for (int64_t d = -(1 << 24); d <= (1 << 24); ++d) // every double within 2^24 ulp of 1.0
        check_pair(from_bits(one + d));
    const int e_lo = -500, e_hi = 500; // the window's exponents
    for (int e = e_lo - 3; e <= e_hi + 3; ++e) // (three binades beyond each edge: slow path)
        for (uint64_t sig : {0x000fffffffffffffull, 0x000ffffffffffffeull, 0ull, 1ull})
            for (int rep = 0; rep < 4; ++rep)
                check_pair(make(sig, e));
    for (int i = 0; i < 2000000; ++i) { // exact squares, and their neighbours
        const uint64_t r = rnd() >> 38; // 26 bits
        const double sq = ldexp((double)(r * r), 2 * ((int)(rnd() % 490) - 245));
        check_pair(sq);
        check_pair(nextafter(sq, 0.0));
        check_pair(nextafter(sq, INFINITY));
    }
    for (int i = 0; i < 50000000; ++i) // random significands over the whole window
        check_pair(make(rnd(), e_lo + (int)(rnd() % 1001)));
    for (int i = 0; i < 2000000; ++i) { // s with an all-ones significand: a = s * s rounded down / to nearest, all exponents
        const double s = make(0x000fffffffffffffull, (int)(rnd() % 500) - 250);
        const double a = s * s;
        check_pair(a);
        check_pair(nextafter(a, 0.0));
        check_pair(nextafter(a, INFINITY));
    }
    const double edges[] = {0x1p-500, 0x1p501, 0.0, -0.0, 0x1p-1074, 0x1p-1022, 0x1.fffffffffffffp1023, INFINITY, -INFINITY, NAN, -1.0, -0x1p-600,
                            0x1p-767, 0x1p-768};
    for (double a : edges) {
        check_pair(a);
        double lo = a, hi = a;
        for (int i = 0; i < 64; ++i) {
            lo = nextafter(lo, -INFINITY);
            hi = nextafter(hi, INFINITY);
            check_pair(lo);
            check_pair(hi);
        }
    }

    // ---- the quotient ----
    double hs[64];
    int n_h = 0;
    for (int k = 1; k <= 39; ++k)
        hs[n_h++] = (1.0 / 60.0) / k;
    for (double h : {1.0 / 60.0, 0.001, 1.0 / 3.0, 1.0 / 1200.0, 1.0 / 420.0, 1.0 / 2340.0, 1.0 / 30.0, 1.0 / 120.0, 0.01, 1.0, 0.5})
        hs[n_h++] = h;
    hs[n_h++] = make(0x000fffffffffffffull, -7);  // all-ones significand: not ok, slow path
    hs[n_h++] = make(0x000ffffffffffffeull, -7);
    hs[n_h++] = 0x1p-64; hs[n_h++] = nextafter(0x1p-64, 0.0); hs[n_h++] = 0x1p64; hs[n_h++] = nextafter(0x1p64, 0.0); // window edges of h
    hs[n_h++] = 0x1p-1040; hs[n_h++] = -1.0 / 60.0; hs[n_h++] = 0.0; hs[n_h++] = INFINITY; hs[n_h++] = NAN;
    const double x_edges[] = {0.0, -0.0, 0x1p-400, -0x1p-400, 0x1p401, -0x1p401, 0x1p-1074, 0x1p-1022, 0x1p-1043, 0x1.fffffffffffffp1023, INFINITY,
                              -INFINITY, NAN};
    for (int j = 0; j < n_h; ++j) {
        const double h = hs[j];
        for (int i = 0; i < 400000; ++i)
            check_div(make(rnd(), (int)(rnd() % 801) - 400, rnd() & 1), h);
        for (double x : x_edges) {
            check_div(x, h);
            double lo = x, hi = x;
            for (int i = 0; i < 16; ++i) {
                lo = nextafter(lo, -INFINITY);
                hi = nextafter(hi, INFINITY);
                check_div(lo, h);
                check_div(hi, h);
            }
        }
        if (h > 0.0 && h < INFINITY && bits_of(h) >> 52 != 0)
            hard_quotients(h);
    }

    printf("pair: %llu operands (%llu fast), %llu root differences, %llu reciprocal differences\n", n_pair, n_pair_fast, bad_root, bad_recip);
    printf("div_by: %llu operands (%llu fast), %llu differences\n", n_div, n_div_fast, bad_div);
    return (bad_root || bad_recip || bad_div) ? 1 : 0;
}
