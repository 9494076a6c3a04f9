// distance_merge_standalone_main.cpp -- the merge of the multi-GPU world's distance queries (merge_first_hits<xpbd_distance_hit>,
// csrc/xpbd_merge.hpp) on hand-made rows, with no device and no Python: built by tests/test_distance_merge_standalone.py with
// plain g++, also under ASan/UBSan.  The expected winner of every query comes from sorting the ranks' records by (distance, body).
// Exits non-zero with a one-line message on the first difference.
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
    std::fprintf(stderr, "distance_merge_standalone: %s: %s (entry %u)\n", scene, what, at);
    return 1;
}

xpbd_distance_hit miss()
{
    xpbd_distance_hit h{};
    h.body = XPBD_NO_HIT, h.index_a = XPBD_NO_HIT, h.index_b = XPBD_NO_HIT, h.distance = INFINITY;
    return h;
}

// An answer of `body` at `distance` whose other fields tell which rank's record it is.
xpbd_distance_hit hit(uint32_t body, double distance, uint32_t rank)
{
    xpbd_distance_hit h{};
    h.body = body, h.feature = rank % 3, h.index_a = rank, h.index_b = body % 7, h.distance = distance;
    for (int a = 0; a < 3; ++a)
        h.point_a[a] = distance + a, h.point_b[a] = (double)body - a, h.normal[a] = (double)rank + a;
    return h;
}

// A body that is not separated from the volume: distance 0, no features, no points.
xpbd_distance_hit overlap(uint32_t body)
{
    xpbd_distance_hit h{};
    h.body = body, h.feature = XPBD_DISTANCE_OVERLAP, h.index_a = XPBD_NO_HIT, h.index_b = XPBD_NO_HIT;
    return h;
}

int check(const char *scene, const std::vector<std::vector<xpbd_distance_hit>> &rows)
{
    const uint32_t n_ranks = (uint32_t)rows.size(), n = (uint32_t)rows[0].size();
    std::vector<xpbd_distance_hit> flat;
    for (const auto &row : rows)
        flat.insert(flat.end(), row.begin(), row.end());
    std::vector<xpbd_distance_hit> got(n);
    xpbd::merge_first_hits<xpbd_distance_hit>(flat.data(), n_ranks, n, got.data());
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<xpbd_distance_hit> all;
        for (const auto &row : rows)
            all.push_back(row[i]);
        std::stable_sort(all.begin(), all.end(), [](const xpbd_distance_hit &a, const xpbd_distance_hit &b) {
            return a.distance != b.distance ? a.distance < b.distance : a.body < b.body;
        });
        if (std::memcmp(&got[i], &all[0], sizeof(xpbd_distance_hit)) != 0)
            return fail(scene, "a query's winner is not the smallest (distance, body)", i);
    }
    return 0;
}

int run()
{
    static_assert(sizeof(xpbd_distance_query) == 80 && sizeof(xpbd_distance_hit) == 96, "xpbd_distance_query is 80 bytes, xpbd_distance_hit 96");
    // by hand: a tie on distance goes to the smaller body wherever it sits; an overlap (0) beats a positive distance; two
    // overlaps tie at 0 and the smaller body wins; a miss loses to anything
    {
        std::vector<std::vector<xpbd_distance_hit>> rows = {{hit(7, 1.5, 0), hit(3, 0.25, 0), overlap(9), miss()},
                                                           {hit(5, 1.5, 1), overlap(8), overlap(4), hit(2, 4.0, 1)}};
        std::vector<xpbd_distance_hit> flat(rows[0]);
        flat.insert(flat.end(), rows[1].begin(), rows[1].end());
        xpbd_distance_hit got[4];
        xpbd::merge_first_hits<xpbd_distance_hit>(flat.data(), 2, 4, got);
        if (got[0].body != 5 || got[0].index_a != 1 || got[0].distance != 1.5)
            return fail("by hand", "a tie on distance did not go to the smaller body", 0);
        if (got[1].body != 8 || got[1].feature != XPBD_DISTANCE_OVERLAP || got[1].distance != 0.0)
            return fail("by hand", "an overlap did not beat a positive distance", 1);
        if (got[2].body != 4 || got[2].feature != XPBD_DISTANCE_OVERLAP)
            return fail("by hand", "two overlaps did not go to the smaller body", 2);
        if (got[3].body != 2 || got[3].distance != 4.0)
            return fail("by hand", "a miss did not lose", 3);
    }
    // exact ties in distance: every rank answers with its own body at one of three distances, 0 among them
    Lcg rng{0x9E3779B97F4A7C15ull};
    const double distances[3] = {0.0, 1.0, 2.0};
    std::vector<std::vector<xpbd_distance_hit>> rows(4, std::vector<xpbd_distance_hit>(257));
    uint32_t ties = 0;
    for (uint32_t i = 0; i < 257; ++i) {
        for (uint32_t r = 0; r < 4; ++r) { // the bodies of a query are distinct, and the lowest is not always on rank 0
            const uint32_t body = 4 * (rng.next() % 1000) + (r + i) % 4;
            const double d = distances[rng.next() % 3];
            rows[r][i] = rng.next() % 5 == 0 ? miss() : (d == 0.0 && rng.next() % 2 ? overlap(body) : hit(body, d, r));
        }
        double least = INFINITY;
        for (uint32_t r = 0; r < 4; ++r)
            least = std::min(least, rows[r][i].distance);
        uint32_t at_least = 0;
        for (uint32_t r = 0; r < 4; ++r)
            at_least += rows[r][i].distance == least && least < INFINITY;
        ties += at_least > 1;
    }
    if (ties < 32)
        return fail("ties", "the case holds too few ties to mean anything", ties);
    if (int rc = check("ties", rows))
        return rc;
    // a rank that finds nothing at all, first and in the middle
    for (uint32_t silent : {0u, 2u}) {
        std::vector<std::vector<xpbd_distance_hit>> some = rows;
        std::fill(some[silent].begin(), some[silent].end(), miss());
        if (int rc = check("a rank without hits", some))
            return rc;
    }
    // everybody misses: the miss record comes through as it is
    std::vector<std::vector<xpbd_distance_hit>> none(3, std::vector<xpbd_distance_hit>(5, miss()));
    if (int rc = check("all miss", none))
        return rc;
    // one rank: its row as it is
    std::vector<xpbd_distance_hit> got(257);
    xpbd::merge_first_hits<xpbd_distance_hit>(rows[1].data(), 1, 257, got.data());
    if (std::memcmp(got.data(), rows[1].data(), 257 * sizeof(xpbd_distance_hit)) != 0)
        return fail("one rank", "the row changed", 0);
    // no queries at all
    xpbd::merge_first_hits<xpbd_distance_hit>(rows[1].data(), 4, 0, got.data());
    return 0;
}

} // namespace

int main()
{
    if (int rc = run())
        return rc;
    std::printf("distance_merge_standalone ok\n");
    return 0;
}
