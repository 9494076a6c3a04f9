// fma_double_add_host.cpp -- host check of the identity behind rotate_bounded (constraint_solver_amd/csrc/xpbd_step.hpp):
//     fma(c, 2.0, v) == c * 2.0 + v   bit for bit, for EVERY c, whenever |v| <= 2^970
// (built and run by tests/test_fma_double_add_host.py with g++ -O2 -ffp-contract=off).  Doubling is exact, so both forms round
// the same real number unless 2c overflows; then the plain form is +-inf, and 2c + v lies at or beyond 2^1024 - 2^970, from
// where rounding to nearest gives +-inf too.  The program walks c over all exponents, over [2^1022, max], subnormals, zeros,
// infinities and NaN, against v of both signs up to the bound, prints the counts, shows that the identity FAILS at
// |v| = 2^971 (so the bound matters), and exits 0 only with zero differences.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t bits_of(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
static double from_bits(uint64_t u)
{
    double x;
    memcpy(&x, &u, 8);
    return x;
}
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() // xorshift64*
{
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}
static double make(uint64_t significand52, int exponent, bool negative)
{
    return from_bits(((uint64_t)negative << 63) | ((uint64_t)(exponent + 1023) << 52) | (significand52 & 0x000fffffffffffffull));
}
static bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

// Kept out of line: the two forms are compiled once each, as written, and meet only through their results.
static __attribute__((noinline)) double plain(double c, double v) { return c * 2.0 + v; }
static __attribute__((noinline)) double fused(double c, double v) { return __builtin_fma(c, 2.0, v); }

static unsigned long long n_checked = 0, n_overflow = 0, n_bad = 0;

static void check(double c, double v)
{
    const double p = plain(c, v), f = fused(c, v);
    ++n_checked;
    n_overflow += std::isfinite(c) && std::isinf(c * 2.0);
    if (!same(p, f) && n_bad++ < 10)
        printf("differ: c=%a v=%a plain %a fused %a\n", c, v, p, f);
}

int main()
{
    const double k2p970 = 0x1p970, below = from_bits(bits_of(k2p970) - 1);
    // addends: what a shape table holds (zeros of both signs, cube and cuboid coordinates), the bound, the values next to
    // it, and random ones of every exponent up to it
    std::vector<double> vs = {0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 0.3, -2.75, 0x1p-1074, -0x1p-1074, 0x1p-1022, 0x1p969, -0x1p969,
                              below, -below, k2p970, -k2p970};
    for (int k = 0; k < 48; ++k)
        vs.push_back(make(rnd(), (int)(rnd() % (970 + 1022)) - 1022, rnd() & 1)); // exponents -1022 .. 969
    for (int k = 0; k < 8; ++k)
        vs.push_back(make(rnd(), 969, rnd() & 1));
    std::vector<double> specials = {0.0, -0.0, INFINITY, -INFINITY, NAN, -NAN, 0x1p1023, -0x1p1023, 0x1.fffffffffffffp1023,
                                    -0x1.fffffffffffffp1023, 0x1.fffffffffffffp1022, -0x1.fffffffffffffp1022, 0x1p1022, -0x1p1022,
                                    0x1p-1074, -0x1p-1074, 0x0.fffffffffffffp-1022, 0x1p-1022, 0x1p-1023};
    for (double v : vs) {
        for (double c : specials)
            check(c, v);
        for (int k = 0; k < 200000; ++k) // every exponent, subnormals (biased exponent 0) included
            check(from_bits((rnd() & 0x800fffffffffffffull) | ((rnd() % 2047) << 52)), v);
        for (int k = 0; k < 100000; ++k) // |c| in [2^1022, max]: half of them overflow when doubled
            check(make(rnd(), 1022 + (int)(rnd() & 1), rnd() & 1), v);
        for (int k = 0; k < 20000; ++k) // subnormal c
            check(from_bits(rnd() & 0x800fffffffffffffull), v);
        for (int k = 0; k < 20000; ++k) // c of v's own size and opposite sign: cancellation
            check(-0.5 * v * (1.0 + (double)(int64_t)(rnd() >> 40) * 0x1p-40), v);
    }
    // 2^1023 * 2 overflows in the plain form, yet 2^1024 - 2^971 is the largest double: the identity needs the bound
    const double c = 0x1p1023, v = -0x1p971;
    const bool counter_example = std::isinf(plain(c, v)) && fused(c, v) == 0x1.fffffffffffffp1023;
    // ... and at the bound itself the sum is the midpoint between that double and 2^1024: ties to even, +inf in both
    const bool tie_at_bound = std::isinf(plain(c, -k2p970)) && std::isinf(fused(c, -k2p970));
    printf("fma_double_add: %llu pairs (%llu with 2c overflowing), %llu differences; counter-example at 2^971: %s; tie at 2^970: %s\n",
           n_checked, n_overflow, n_bad, counter_example ? "yes" : "NO", tie_at_bound ? "inf" : "NOT inf");
    return n_bad == 0 && counter_example && tie_at_bound ? 0 : 1;
}
