// sweep_merge_standalone_main.cpp -- the merge of the multi-GPU world's sweep queries (merge_first_hits<xpbd_sweep_hit>,
// csrc/xpbd_merge.hpp) on hand-made rows, with no device and no Python: built by tests/test_sweep_merge_standalone.py with plain g++, also under
// ASan/UBSan.  The expected winner of every sweep comes from sorting the ranks' records by (distance, body).  Exits non-zero with
// a one-line message on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_merge.hpp"

namespace {

struct Lcg { // Knuth's MMIX constants; the high bits
    uint64_t state;
    uint32_t next() { return (uint32_t)((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
};

int fail(const char *scene, const char *what, uint32_t at)
{
    std::fprintf(stderr, "sweep_merge_standalone: %s: %s (entry %u)\n", scene, what, at);
    return 1;
}

xpbd_sweep_hit miss()
{
    xpbd_sweep_hit h{};
    h.body = XPBD_NO_HIT, h.face = XPBD_NO_HIT, h.distance = INFINITY;
    return h;
}

// A hit of `body` at `distance` whose other fields tell which rank's record it is.
xpbd_sweep_hit hit(uint32_t body, double distance, uint32_t rank)
{
    xpbd_sweep_hit h{};
    h.body = body, h.feature = rank % 4, h.face = rank, h.distance = distance;
    for (int a = 0; a < 3; ++a)
        h.position[a] = distance + a, h.normal[a] = (double)body - a;
    return h;
}

int check(const char *scene, const std::vector<std::vector<xpbd_sweep_hit>> &rows)
{
    const uint32_t n_ranks = (uint32_t)rows.size(), n = (uint32_t)rows[0].size();
    std::vector<xpbd_sweep_hit> flat;
    for (const auto &row : rows)
        flat.insert(flat.end(), row.begin(), row.end());
    std::vector<xpbd_sweep_hit> got(n);
    xpbd::merge_first_hits<xpbd_sweep_hit>(flat.data(), n_ranks, n, got.data());
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<xpbd_sweep_hit> all;
        for (const auto &row : rows)
            all.push_back(row[i]);
        std::stable_sort(all.begin(), all.end(), [](const xpbd_sweep_hit &a, const xpbd_sweep_hit &b) {
            return a.distance != b.distance ? a.distance < b.distance : a.body < b.body;
        });
        if (std::memcmp(&got[i], &all[0], sizeof(xpbd_sweep_hit)) != 0)
            return fail(scene, "a sweep's winner is not the smallest (distance, body)", i);
    }
    return 0;
}

int run()
{
    static_assert(sizeof(xpbd_sweep) == 104 && sizeof(xpbd_sweep_hit) == 72, "xpbd_sweep is 104 bytes, xpbd_sweep_hit 72");
    // by hand: two ranks tie at distance 0 (initial overlaps), the smaller body wins wherever it sits
    {
        std::vector<std::vector<xpbd_sweep_hit>> rows = {{hit(7, 0.0, 0), hit(3, 1.5, 0), miss()}, {hit(5, 0.0, 1), hit(9, 1.5, 1), hit(2, 4.0, 1)}};
        std::vector<xpbd_sweep_hit> flat(rows[0]);
        flat.insert(flat.end(), rows[1].begin(), rows[1].end());
        xpbd_sweep_hit got[3];
        xpbd::merge_first_hits<xpbd_sweep_hit>(flat.data(), 2, 3, got);
        if (got[0].body != 5 || got[0].face != 1 || got[1].body != 3 || got[1].face != 0 || got[2].body != 2 || got[2].distance != 4.0)
            return fail("sweeps, by hand", "wrong winner", 0);
    }
    // exact ties in distance: every rank hits its own body at one of three distances
    Lcg rng{0x9E3779B97F4A7C15ull};
    const double distances[3] = {0.0, 1.0, 2.0};
    std::vector<std::vector<xpbd_sweep_hit>> rows(4, std::vector<xpbd_sweep_hit>(257));
    uint32_t ties = 0;
    for (uint32_t i = 0; i < 257; ++i) {
        for (uint32_t r = 0; r < 4; ++r) // the bodies of a sweep are distinct, and the lowest is not always on rank 0
            rows[r][i] = rng.next() % 5 == 0 ? miss() : hit(4 * (rng.next() % 1000) + (r + i) % 4, distances[rng.next() % 3], r);
        double least = INFINITY;
        for (uint32_t r = 0; r < 4; ++r)
            least = std::min(least, rows[r][i].distance);
        uint32_t at_least = 0;
        for (uint32_t r = 0; r < 4; ++r)
            at_least += rows[r][i].distance == least && least < INFINITY;
        ties += at_least > 1;
    }
    if (ties < 32)
        return fail("sweeps, ties", "the case holds too few ties to mean anything", ties);
    if (int rc = check("sweeps, ties", rows))
        return rc;
    // a rank that hits nothing at all, first and in the middle
    for (uint32_t silent : {0u, 2u}) {
        std::vector<std::vector<xpbd_sweep_hit>> some = rows;
        std::fill(some[silent].begin(), some[silent].end(), miss());
        if (int rc = check("sweeps, a rank without hits", some))
            return rc;
    }
    // everybody misses: the miss record comes through as it is
    std::vector<std::vector<xpbd_sweep_hit>> none(3, std::vector<xpbd_sweep_hit>(5, miss()));
    if (int rc = check("sweeps, all miss", none))
        return rc;
    // one rank: its row as it is
    std::vector<xpbd_sweep_hit> got(257);
    xpbd::merge_first_hits<xpbd_sweep_hit>(rows[1].data(), 1, 257, got.data());
    if (std::memcmp(got.data(), rows[1].data(), 257 * sizeof(xpbd_sweep_hit)) != 0)
        return fail("sweeps, one rank", "the row changed", 0);
    // no sweeps at all
    xpbd::merge_first_hits<xpbd_sweep_hit>(rows[1].data(), 4, 0, got.data());
    return 0;
}

} // namespace

int main()
{
    if (int rc = run())
        return rc;
    std::printf("sweep_merge_standalone ok\n");
    return 0;
}
