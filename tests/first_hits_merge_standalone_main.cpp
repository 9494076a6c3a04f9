// first_hits_merge_standalone_main.cpp -- merge_first_hits (csrc/xpbd_merge.hpp) instantiated for the three records it serves
// (xpbd_ray_hit, xpbd_sweep_hit, xpbd_distance_hit) over the SAME (distance, body) rows, with no device and no Python: built by
// tests/test_first_hits_merge_standalone.py with plain g++, also under ASan/UBSan.  The winners are written down by hand, every
// record type must name them, and so the three agree.  Exits non-zero with a one-line message on the first difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_merge.hpp"

namespace {

struct Entry {
    double distance;
    uint32_t body;
};
const Entry kMiss{INFINITY, XPBD_NO_HIT};

constexpr uint32_t kRanks = 3, kQueries = 5;
// rank x query: a tie on distance that the body decides (the smaller body on the LAST rank), the same tie the other way round,
// a plain minimum in the middle, one hit among misses, and misses all round.
const Entry kRows[kRanks][kQueries] = {
    {{1.5, 9}, {0.0, 2}, {4.0, 1}, kMiss, kMiss},
    {{2.5, 0}, {0.0, 7}, {0.25, 6}, kMiss, kMiss},
    {{1.5, 4}, {0.5, 0}, {0.5, 3}, {8.0, 5}, kMiss},
};
const Entry kWinners[kQueries] = {{1.5, 4}, {0.0, 2}, {0.25, 6}, {8.0, 5}, kMiss};
const uint32_t kWinnerRank[kQueries] = {2, 0, 1, 2, 0}; // (all misses: the first rank's record as it is)

// A record of type Hit for `e` whose every other byte tells which rank and query it came from.
template <class Hit>
Hit record(const Entry &e, uint32_t rank, uint32_t query)
{
    Hit h;
    std::memset(&h, (int)(0x10 * (rank + 1) + query), sizeof h);
    h.distance = e.distance;
    h.body = e.body;
    return h;
}

template <class Hit>
int run(const char *type, std::vector<Entry> &winners)
{
    std::vector<Hit> flat;
    for (uint32_t r = 0; r < kRanks; ++r)
        for (uint32_t q = 0; q < kQueries; ++q)
            flat.push_back(record<Hit>(kRows[r][q], r, q));
    std::vector<Hit> got(kQueries);
    xpbd::merge_first_hits<Hit>(flat.data(), kRanks, kQueries, got.data());
    for (uint32_t q = 0; q < kQueries; ++q) {
        const Hit want = record<Hit>(kRows[kWinnerRank[q]][q], kWinnerRank[q], q); // the whole record of the winning rank
        if (std::memcmp(&got[q], &want, sizeof(Hit)) != 0 || std::memcmp(&got[q].distance, &kWinners[q].distance, sizeof(double)) != 0 ||
            got[q].body != kWinners[q].body) {
            std::fprintf(stderr, "first_hits_merge_standalone: %s: query %u: got (%g, %u)\n", type, q, got[q].distance, got[q].body);
            return 1;
        }
        winners.push_back(Entry{got[q].distance, got[q].body});
    }
    // one rank: its row as it is (the last one, so an offset by rank would show)
    std::vector<Hit> one(kQueries);
    xpbd::merge_first_hits<Hit>(flat.data() + 2 * kQueries, 1, kQueries, one.data());
    if (std::memcmp(one.data(), flat.data() + 2 * kQueries, kQueries * sizeof(Hit)) != 0) {
        std::fprintf(stderr, "first_hits_merge_standalone: %s: one rank: the row changed\n", type);
        return 1;
    }
    // no queries: nothing is read and nothing written, whatever the number of ranks
    Hit untouched = record<Hit>(kMiss, 7, 7), before = untouched;
    xpbd::merge_first_hits<Hit>(nullptr, kRanks, 0, &untouched);
    if (std::memcmp(&untouched, &before, sizeof(Hit)) != 0) {
        std::fprintf(stderr, "first_hits_merge_standalone: %s: n == 0 wrote a record\n", type);
        return 1;
    }
    return 0;
}

} // namespace

int main()
{
    std::vector<Entry> of_rays, of_sweeps, of_distances;
    if (run<xpbd_ray_hit>("xpbd_ray_hit", of_rays) || run<xpbd_sweep_hit>("xpbd_sweep_hit", of_sweeps) ||
        run<xpbd_distance_hit>("xpbd_distance_hit", of_distances))
        return 1;
    for (uint32_t q = 0; q < kQueries; ++q) {
        const bool agree = std::memcmp(&of_rays[q].distance, &of_sweeps[q].distance, sizeof(double)) == 0 &&
                           std::memcmp(&of_rays[q].distance, &of_distances[q].distance, sizeof(double)) == 0 &&
                           of_rays[q].body == of_sweeps[q].body && of_rays[q].body == of_distances[q].body;
        if (!agree) {
            std::fprintf(stderr, "first_hits_merge_standalone: query %u: the three record types name different winners\n", q);
            return 1;
        }
        std::printf("winner %u: %g %u\n", q, of_rays[q].distance, of_rays[q].body);
    }
    std::printf("first_hits_merge_standalone ok\n");
    return 0;
}
