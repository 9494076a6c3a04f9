// plan_standalone_main.cpp -- the shard planner (csrc/xpbd_plan.cpp + csrc/xpbd_error.cpp) on its own, with no device and no
// Python: built by tests/test_plan_standalone.py with plain g++, also under ASan/UBSan and TSan.  Exits non-zero with a
// one-line message on the first difference.  Same properties as tests/test_halo_plan_native.py, through the C ABI.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/xpbd.h"

namespace {

struct Lcg { // Knuth's MMIX constants; the high bits
    uint64_t state;
    uint32_t next() { return (uint32_t)((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
    double uniform() { return (double)next() / 2147483648.0; } // [0, 1)
};

struct Scene {
    const char *name;
    uint32_t n;
    double edge, extent[3]; // the bodies' centres: uniform in a box of this size
};

int fail(const Scene &s, uint32_t n_ranks, const char *what, uint32_t rank, uint32_t at)
{
    std::fprintf(stderr, "plan_standalone: %s, %u ranks: %s (rank %u, entry %u) -- %s\n", s.name, n_ranks, what, rank, at, xpbd_last_error());
    return 1;
}

int run(const Scene &s)
{
    const uint32_t n = s.n, n_joints = 40;
    Lcg rng{0x9E3779B97F4A7C15ull ^ n};
    // cell keys at the cut, and after every body has moved by less than one cell along every axis
    std::vector<int64_t> k0(n), k1(n);
    for (uint32_t g = 0; g < n; ++g) {
        double c0[3], c1[3];
        for (int a = 0; a < 3; ++a) {
            c0[a] = rng.uniform() * s.extent[a];
            c1[a] = c0[a] + (rng.uniform() - 0.5) * 1.96 * s.edge;
        }
        k0[g] = xpbd_halo_cell_key(c0, s.edge);
        k1[g] = xpbd_halo_cell_key(c1, s.edge);
    }
    std::vector<xpbd_joint> joints(n_joints, xpbd_joint{}); // random bodies up to 200 ids apart: many cross shard boundaries
    for (xpbd_joint &j : joints) {
        j.body_a = rng.next() % (n - 200);
        j.body_b = j.body_a + 1 + rng.next() % 199;
    }
    for (uint32_t w : {2u, 3u, 5u}) {
        // 1. ownership is a function of the keys alone
        std::vector<uint8_t> owner(n), again(n);
        if (xpbd_halo_partition(k0.data(), n, w, owner.data()) || xpbd_halo_partition(k0.data(), n, w, again.data()))
            return fail(s, w, "xpbd_halo_partition failed", 0, 0);
        for (uint32_t g = 0; g < n; ++g)
            if (owner[g] != again[g] || owner[g] >= w)
                return fail(s, w, "the owners of a second call differ", owner[g], g);
        // 2. a body is on its owner's boundary list iff another rank lists it as a ghost
        std::vector<uint8_t> on_boundary(n, 0), mirrored(n, 0), far(n);
        std::vector<uint32_t> ghosts(n), boundary(n);
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t n_ghosts = 0, n_boundary = 0;
            if (xpbd_halo_plan_owned(k0.data(), owner.data(), n, w, r, joints.data(), n_joints, ghosts.data(), &n_ghosts, boundary.data(), &n_boundary,
                                     nullptr, n))
                return fail(s, w, "xpbd_halo_plan_owned failed", r, 0);
            for (uint32_t i = 0; i < n_ghosts; ++i) {
                if (ghosts[i] >= n || owner[ghosts[i]] == r)
                    return fail(s, w, "a rank mirrors a body of its own", r, i);
                mirrored[ghosts[i]] = 1;
            }
            for (uint32_t i = 0; i < n_boundary; ++i) {
                if (boundary[i] >= n || owner[boundary[i]] != r)
                    return fail(s, w, "a boundary body is not the rank's", r, i);
                on_boundary[boundary[i]] = 1;
            }
        }
        for (uint32_t g = 0; g < n; ++g)
            if (on_boundary[g] != mirrored[g])
                return fail(s, w, "boundary lists and ghost lists disagree", owner[g], g);
        // 3. the light plan after the motion == the full planner with the owners the light plan reports
        std::vector<uint8_t> owner_now(n), far_light(n);
        std::vector<uint32_t> own(n), ghosts_light(n), boundary_light(n);
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t n_own = 0, n_ghosts_light = 0, n_boundary_light = 0, n_ghosts = 0, n_boundary = 0;
            if (xpbd_halo_plan_light(k0.data(), k1.data(), n, w, r, joints.data(), n_joints, owner_now.data(), own.data(), &n_own, ghosts_light.data(),
                                     &n_ghosts_light, boundary_light.data(), &n_boundary_light, far_light.data(), n))
                return fail(s, w, "xpbd_halo_plan_light failed", r, 0);
            if (xpbd_halo_plan_owned(k1.data(), owner_now.data(), n, w, r, joints.data(), n_joints, ghosts.data(), &n_ghosts, boundary.data(), &n_boundary,
                                     far.data(), n))
                return fail(s, w, "xpbd_halo_plan_owned failed after the motion", r, 0);
            uint32_t k = 0;
            for (uint32_t g = 0; g < n; ++g)
                if (owner_now[g] == r && (k >= n_own || own[k++] != g))
                    return fail(s, w, "light plan: `own` is not the bodies the rank owns now", r, g);
            if (k != n_own || n_ghosts_light != n_ghosts || n_boundary_light != n_boundary)
                return fail(s, w, "light plan: list lengths differ from the full planner's", r, n_own);
            for (uint32_t i = 0; i < n_ghosts; ++i)
                if (ghosts_light[i] != ghosts[i])
                    return fail(s, w, "light plan: ghosts differ", r, i);
            for (uint32_t i = 0; i < n_boundary; ++i)
                if (boundary_light[i] != boundary[i])
                    return fail(s, w, "light plan: boundary differs", r, i);
            for (uint32_t i = 0; i < n_own; ++i)
                if (far_light[i] != far[i])
                    return fail(s, w, "light plan: far flags differ", r, i);
        }
    }
    return 0;
}

} // namespace

int main()
{
    const double edge = 2.04;
    // 70 001: past the 65 536 bodies above which the planner's passes run in threads, in uneven chunks
    const Scene scenes[] = {{"cloud of 997", 997, edge, {12.0, 12.0, 12.0}}, {"slab of 70001", 70001, edge, {64 * edge, 8 * edge, 8 * edge}}};
    for (const Scene &s : scenes)
        if (int rc = run(s))
            return rc;
    std::puts("plan_standalone: ok");
    return 0;
}
