// merge_standalone_main.cpp -- the merges of the multi-GPU world's scene queries and contact reports (csrc/xpbd_merge.hpp) on
// their own, with no device and no Python: built by tests/test_merge_standalone.py with plain g++, also under ASan/UBSan.  The
// expected answers come from concatenating every rank's candidates and sorting them, the events from set differences.  Exits
// non-zero with a one-line message on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_merge.hpp"

namespace {

struct Lcg { // Knuth's MMIX constants; the high bits
    uint64_t state;
    uint32_t next() { return (uint32_t)((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
};

int fail(const char *scene, const char *what, uint32_t at)
{
    std::fprintf(stderr, "merge_standalone: %s: %s (entry %u)\n", scene, what, at);
    return 1;
}

// ---- ray casts -------------------------------------------------------------------------------------------------------------
xpbd_ray_hit miss()
{
    xpbd_ray_hit h{};
    h.body = XPBD_NO_HIT, h.face = XPBD_NO_HIT, h.distance = INFINITY;
    return h;
}

// A hit of `body` at `distance` whose other fields tell which rank's record it is.
xpbd_ray_hit hit(uint32_t body, double distance, uint32_t rank)
{
    xpbd_ray_hit h{};
    h.body = body, h.face = rank, h.distance = distance;
    for (int a = 0; a < 3; ++a)
        h.point[a] = distance + a, h.normal[a] = (double)body - a;
    return h;
}

int check_rays(const char *scene, const std::vector<std::vector<xpbd_ray_hit>> &rows)
{
    const uint32_t n_ranks = (uint32_t)rows.size(), n_rays = (uint32_t)rows[0].size();
    std::vector<xpbd_ray_hit> flat;
    for (const auto &row : rows)
        flat.insert(flat.end(), row.begin(), row.end());
    std::vector<xpbd_ray_hit> got(n_rays);
    xpbd::merge_first_hits<xpbd_ray_hit>(flat.data(), n_ranks, n_rays, got.data());
    for (uint32_t i = 0; i < n_rays; ++i) {
        std::vector<xpbd_ray_hit> all;
        for (const auto &row : rows)
            all.push_back(row[i]);
        std::stable_sort(all.begin(), all.end(), [](const xpbd_ray_hit &a, const xpbd_ray_hit &b) {
            return a.distance != b.distance ? a.distance < b.distance : a.body < b.body;
        });
        if (std::memcmp(&got[i], &all[0], sizeof(xpbd_ray_hit)) != 0)
            return fail(scene, "a ray's winner is not the smallest (distance, body)", i);
    }
    return 0;
}

int run_rays()
{
    // exact ties in distance: every rank hits its own body at one of three distances
    Lcg rng{0x9E3779B97F4A7C15ull};
    const double distances[3] = {0.5, 1.0, 2.0};
    std::vector<std::vector<xpbd_ray_hit>> rows(4, std::vector<xpbd_ray_hit>(257));
    uint32_t ties = 0;
    for (uint32_t i = 0; i < 257; ++i) {
        for (uint32_t r = 0; r < 4; ++r) // the bodies of a ray are distinct, and the lowest is not always on rank 0
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
        return fail("rays, ties", "the case holds too few ties to mean anything", ties);
    if (int rc = check_rays("rays, ties", rows))
        return rc;
    // a rank that hits nothing at all, first and in the middle
    for (uint32_t silent : {0u, 2u}) {
        std::vector<std::vector<xpbd_ray_hit>> some = rows;
        std::fill(some[silent].begin(), some[silent].end(), miss());
        if (int rc = check_rays("rays, a rank without hits", some))
            return rc;
    }
    // everybody misses
    std::vector<std::vector<xpbd_ray_hit>> none(3, std::vector<xpbd_ray_hit>(5, miss()));
    if (int rc = check_rays("rays, all miss", none))
        return rc;
    // one rank: its row as it is
    std::vector<std::vector<xpbd_ray_hit>> one(rows.begin() + 1, rows.begin() + 2);
    if (int rc = check_rays("rays, one rank", one))
        return rc;
    std::vector<xpbd_ray_hit> got(257);
    xpbd::merge_first_hits<xpbd_ray_hit>(one[0].data(), 1, 257, got.data());
    if (std::memcmp(got.data(), one[0].data(), 257 * sizeof(xpbd_ray_hit)) != 0)
        return fail("rays, one rank", "the row changed", 0);
    return 0;
}

// ---- overlap queries -------------------------------------------------------------------------------------------------------
using Lists = std::vector<std::vector<std::vector<xpbd_overlap_hit>>>; // [rank][query]: that rank's hits of that query

xpbd_overlap_hit overlap_hit(uint32_t body, uint32_t rank) { return xpbd_overlap_hit{body, rank, -1.0 - (double)body / 1024.0}; }

// `expected`: the merged list of every query; the merge is run with every cap from 0 to a few past the total.
int check_overlaps(const char *scene, const Lists &lists, const std::vector<std::vector<xpbd_overlap_hit>> &expected)
{
    const uint32_t n_ranks = (uint32_t)lists.size(), n_queries = (uint32_t)expected.size();
    uint32_t widest = 1;
    for (const auto &rank : lists) {
        size_t total = 0;
        for (const auto &l : rank)
            total += l.size();
        widest = std::max<uint32_t>(widest, (uint32_t)total);
    }
    // the gathered rows; the padding past a rank's list holds a pattern that is no valid hit
    std::vector<uint32_t> offset_rows;
    std::vector<xpbd_overlap_hit> hit_rows((size_t)n_ranks * widest);
    std::memset(hit_rows.data(), 0xEE, hit_rows.size() * sizeof(xpbd_overlap_hit));
    for (uint32_t r = 0; r < n_ranks; ++r) {
        uint32_t at = 0;
        for (uint32_t q = 0; q < n_queries; ++q) {
            offset_rows.push_back(at);
            for (const xpbd_overlap_hit &h : lists[r][q])
                hit_rows[(size_t)r * widest + at++] = h;
        }
        offset_rows.push_back(at);
    }
    std::vector<xpbd_overlap_hit> flat;
    std::vector<uint32_t> want_offsets;
    for (const auto &l : expected) {
        want_offsets.push_back((uint32_t)flat.size());
        flat.insert(flat.end(), l.begin(), l.end());
    }
    want_offsets.push_back((uint32_t)flat.size());
    const uint32_t total = (uint32_t)flat.size();
    for (uint32_t cap = 0; cap <= total + 2; ++cap) {
        std::vector<uint32_t> offsets((size_t)n_queries + 1, 0xABABABABu);
        std::vector<xpbd_overlap_hit> hits((size_t)cap + 4);
        std::memset(hits.data(), 0xCD, hits.size() * sizeof(xpbd_overlap_hit));
        const std::vector<xpbd_overlap_hit> guard = hits;
        const uint32_t got = xpbd::merge_overlap_lists(offset_rows.data(), hit_rows.data(), widest, n_ranks, n_queries, offsets.data(),
                                                       cap ? hits.data() : nullptr, cap);
        if (got != total)
            return fail(scene, "the total does not run past cap to the number of hits", cap);
        if (offsets != want_offsets)
            return fail(scene, "an offset is wrong", cap);
        const uint32_t held = std::min(total, cap);
        if (held && std::memcmp(hits.data(), flat.data(), (size_t)held * sizeof(xpbd_overlap_hit)) != 0)
            return fail(scene, "the hits up to cap are not the first entries of the merged list", cap);
        if (std::memcmp(hits.data() + held, guard.data() + held, (hits.size() - held) * sizeof(xpbd_overlap_hit)) != 0)
            return fail(scene, "something was written past cap", cap);
    }
    return 0;
}

// Concatenate the ranks' lists of every query and sort by body.
std::vector<std::vector<xpbd_overlap_hit>> concatenate_and_sort(const Lists &lists)
{
    std::vector<std::vector<xpbd_overlap_hit>> out(lists[0].size());
    for (size_t q = 0; q < out.size(); ++q) {
        for (const auto &rank : lists)
            out[q].insert(out[q].end(), rank[q].begin(), rank[q].end());
        std::sort(out[q].begin(), out[q].end(), [](const xpbd_overlap_hit &a, const xpbd_overlap_hit &b) { return a.body < b.body; });
    }
    return out;
}

int run_overlaps()
{
    // by hand: three ranks, six queries; body b belongs to rank b % 3
    auto list = [](uint32_t rank, std::initializer_list<uint32_t> bodies) {
        std::vector<xpbd_overlap_hit> l;
        for (uint32_t b : bodies)
            l.push_back(overlap_hit(b, rank));
        return l;
    };
    Lists hand(3, std::vector<std::vector<xpbd_overlap_hit>>(6));
    hand[1][0] = list(1, {22, 4, 13, 7});        // one rank only, and not ascending: it must come out as it is
    hand[0][1] = list(0, {3, 9, 30});            // three ranks
    hand[1][1] = list(1, {1, 10, 28, 31});
    hand[2][1] = list(2, {2, 5, 29});
    //   [.][2] and [.][3]: nobody
    hand[2][4] = list(2, {8, 11});               // two ranks, the higher rank first in body order
    hand[0][4] = list(0, {12});
    //   [.][5]: nobody, at the end
    std::vector<std::vector<xpbd_overlap_hit>> want = concatenate_and_sort(hand);
    want[0] = hand[1][0];
    const uint32_t ascending[] = {1, 2, 3, 5, 9, 10, 28, 29, 30, 31};
    for (size_t i = 0; i < 10; ++i)
        if (want[1].size() != 10 || want[1][i].body != ascending[i] || want[1][i].feature != ascending[i] % 3)
            return fail("overlaps, by hand", "the test's own expectation is wrong", (uint32_t)i);
    if (int rc = check_overlaps("overlaps, by hand", hand, want))
        return rc;
    // random: ascending lists of 0 .. 5 bodies per rank and query, half of the queries empty on a given rank
    for (uint32_t n_ranks : {1u, 2u, 4u}) {
        Lcg rng{0xD1B54A32D192ED03ull ^ n_ranks};
        Lists lists(n_ranks, std::vector<std::vector<xpbd_overlap_hit>>(41));
        for (uint32_t r = 0; r < n_ranks; ++r)
            for (auto &l : lists[r]) {
                uint32_t body = r;
                for (uint32_t k = rng.next() % 2 ? rng.next() % 6 : 0; k > 0; --k)
                    l.push_back(overlap_hit(body += n_ranks * (1 + rng.next() % 7), r));
            }
        if (int rc = check_overlaps("overlaps, random", lists, concatenate_and_sort(lists)))
            return rc;
    }
    // no hits at all: widest is 1, cap = 0 with NULL hits among the caps
    Lists nothing(2, std::vector<std::vector<xpbd_overlap_hit>>(3));
    return check_overlaps("overlaps, no hits", nothing, concatenate_and_sort(nothing));
}

// ---- contact reports -------------------------------------------------------------------------------------------------------
struct RankReport {
    std::vector<xpbd_pair_contact> pairs; // in the rank's own key order
    std::vector<xpbd_contact_point> points;
};

int check_report(const char *scene, const std::vector<RankReport> &ranks, const std::vector<uint64_t> &prev)
{
    const uint32_t n_ranks = (uint32_t)ranks.size();
    uint32_t pair_width = 1, point_width = 1;
    std::vector<uint32_t> counts;
    for (const RankReport &r : ranks) {
        pair_width = std::max(pair_width, (uint32_t)r.pairs.size());
        point_width = std::max(point_width, (uint32_t)r.points.size());
        counts.push_back((uint32_t)r.pairs.size());
    }
    // the gathered rows; the padding holds a pattern that is no record
    std::vector<xpbd_pair_contact> pair_rows((size_t)n_ranks * pair_width);
    std::vector<xpbd_contact_point> point_rows((size_t)n_ranks * point_width);
    std::memset(pair_rows.data(), 0xEE, pair_rows.size() * sizeof(xpbd_pair_contact));
    std::memset(point_rows.data(), 0xEE, point_rows.size() * sizeof(xpbd_contact_point));
    struct Want {
        uint64_t key;
        xpbd_pair_contact pair;
        std::vector<xpbd_contact_point> points;
    };
    std::vector<Want> want;
    for (uint32_t r = 0; r < n_ranks; ++r) {
        std::copy(ranks[r].pairs.begin(), ranks[r].pairs.end(), pair_rows.begin() + (size_t)r * pair_width);
        std::copy(ranks[r].points.begin(), ranks[r].points.end(), point_rows.begin() + (size_t)r * point_width);
        for (const xpbd_pair_contact &c : ranks[r].pairs)
            want.push_back(Want{(uint64_t)c.body_a << 32 | c.body_b, c,
                                std::vector<xpbd_contact_point>(ranks[r].points.begin() + c.first_point, ranks[r].points.begin() + c.first_point + c.n_points)});
    }
    std::sort(want.begin(), want.end(), [](const Want &a, const Want &b) { return a.key < b.key; });
    std::vector<xpbd_pair_contact> pairs(3); // (whatever the vectors held is replaced)
    std::vector<xpbd_contact_point> points(5);
    std::vector<uint64_t> keys(7);
    xpbd::merge_contact_reports(pair_rows.data(), pair_width, counts.data(), point_rows.data(), point_width, n_ranks, pairs, points, keys);
    if (pairs.size() != want.size() || keys.size() != want.size())
        return fail(scene, "the merged report has the wrong number of pairs", (uint32_t)pairs.size());
    uint32_t at = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        xpbd_pair_contact c = want[i].pair;
        c.first_point = at;
        if (keys[i] != want[i].key || std::memcmp(&pairs[i], &c, sizeof c) != 0)
            return fail(scene, "a pair is out of key order or its first_point is not re-based", (uint32_t)i);
        if (points.size() < at + c.n_points ||
            (c.n_points && std::memcmp(&points[at], want[i].points.data(), c.n_points * sizeof(xpbd_contact_point)) != 0))
            return fail(scene, "a pair's points did not follow it", (uint32_t)i);
        at += c.n_points;
    }
    if (points.size() != at)
        return fail(scene, "points nobody refers to", at);
    // events: BEGINs = keys - prev, ENDs = prev - keys, each ascending
    const std::set<uint64_t> now(keys.begin(), keys.end()), before(prev.begin(), prev.end());
    std::vector<xpbd_contact_event> want_events, events(2);
    for (uint64_t k : now)
        if (!before.count(k))
            want_events.push_back(xpbd_contact_event{(uint32_t)(k >> 32), (uint32_t)k, XPBD_CONTACT_BEGIN});
    const uint32_t want_begins = (uint32_t)want_events.size();
    for (uint64_t k : before)
        if (!now.count(k))
            want_events.push_back(xpbd_contact_event{(uint32_t)(k >> 32), (uint32_t)k, XPBD_CONTACT_END});
    const uint32_t begins = xpbd::contact_events(keys, prev, events);
    if (begins != want_begins || events.size() != want_events.size() ||
        (!events.empty() && std::memcmp(events.data(), want_events.data(), events.size() * sizeof(xpbd_contact_event)) != 0))
        return fail(scene, "the events are not the BEGINs then the ENDs of the set differences, in key order", begins);
    return 0;
}

int run_reports()
{
    for (uint32_t n_ranks : {2u, 3u, 4u}) {
        Lcg rng{0xA0761D6478BD642Full ^ n_ranks};
        // disjoint lists: the pair (a, b) belongs to rank a % n_ranks; rank 1 has no pairs; 0 .. 8 points each
        std::vector<RankReport> ranks(n_ranks);
        std::vector<uint64_t> all_keys;
        for (uint32_t r = 0; r < n_ranks; ++r) {
            if (r == 1)
                continue;
            uint32_t a = r;
            for (uint32_t k = 0; k < 37; ++k) {
                a += n_ranks * (rng.next() % 3); // (the same a again: several pairs of one lower body)
                xpbd_pair_contact c{};
                c.body_a = a, c.body_b = a + 1 + 50 * k + rng.next() % 50, c.substeps = 1 + rng.next() % 20, c.n_points = rng.next() % 9;
                c.feature = r, c.first_point = (uint32_t)ranks[r].points.size(), c.depth = -(double)k;
                for (uint32_t q = 0; q < c.n_points; ++q) {
                    xpbd_contact_point p{};
                    p.p_ref[0] = (double)c.body_a, p.p_ref[1] = (double)c.body_b, p.p_inc[2] = (double)q;
                    ranks[r].points.push_back(p);
                }
                ranks[r].pairs.push_back(c);
                all_keys.push_back((uint64_t)c.body_a << 32 | c.body_b);
            }
        }
        // the previous frame: half of this frame's pairs and as many that are gone
        std::vector<uint64_t> prev;
        for (uint64_t k : all_keys) {
            if (rng.next() % 2)
                prev.push_back(k);
            if (rng.next() % 2)
                prev.push_back(k ^ 0x80000000ull); // (body_b + 2^31: no pair of this frame)
        }
        std::sort(prev.begin(), prev.end());
        if (int rc = check_report("reports, random", ranks, prev))
            return rc;
        if (int rc = check_report("reports, empty previous frame", ranks, {}))
            return rc;
        if (int rc = check_report("reports, empty frame", std::vector<RankReport>(n_ranks), prev))
            return rc;
        if (int rc = check_report("reports, nothing at all", std::vector<RankReport>(n_ranks), {}))
            return rc;
    }
    return 0;
}

} // namespace

int main()
{
    if (int rc = run_rays())
        return rc;
    if (int rc = run_overlaps())
        return rc;
    if (int rc = run_reports())
        return rc;
    std::puts("merge_standalone: ok");
    return 0;
}
