// xpbd_merge.hpp -- how the multi-GPU world (xpbd_multi.cpp) merges what its ranks answer: the hits of the scene queries (ray
// casts, sweeps, distances, overlaps) and the contact report of a frame with its begin / end events.  Host-only: pure functions of the
// gathered bytes, no device and no collective (tests/merge_standalone_main.cpp runs them on their own).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xpbd.h"

namespace xpbd {

// rows: n_ranks rows of n records of type Hit (xpbd_ray_hit, xpbd_sweep_hit, xpbd_distance_hit), rank r's answer for its owned
// bodies (a miss: XPBD_NO_HIT at +inf; a distance query's overlap: distance 0, so neither needs a rule of its own).  out[i] = the
// minimum over the ranks under the order of a single world: distance, then body.
template <class Hit>
void merge_first_hits(const void *rows, uint32_t n_ranks, uint32_t n, Hit *out)
{
    const uint8_t *bytes = static_cast<const uint8_t *>(rows);
    for (uint32_t i = 0; i < n; ++i) {
        Hit best;
        std::memcpy(&best, bytes + (size_t)i * sizeof best, sizeof best);
        for (uint32_t r = 1; r < n_ranks; ++r) {
            Hit h;
            std::memcpy(&h, bytes + ((size_t)r * n + i) * sizeof h, sizeof h);
            if (h.distance < best.distance || (h.distance == best.distance && h.body < best.body))
                best = h;
        }
        out[i] = best;
    }
}

// offset_rows: n_ranks rows of n_queries + 1 CSR offsets into the rank's row of hit_rows (n_ranks rows of `widest`
// xpbd_overlap_hit).  The ranks' lists of a query are disjoint and each ascends in body, so a query one rank answers keeps its
// order and the others are sorted.  Writes offsets[0 .. n_queries] and hits[0 .. min(total, cap)) (hits may be NULL with cap ==
// 0); returns the total, counted past cap.
inline uint32_t merge_overlap_lists(const void *offset_rows, const void *hit_rows, uint32_t widest, uint32_t n_ranks, uint32_t n_queries,
                                    uint32_t *offsets, xpbd_overlap_hit *hits, uint32_t cap)
{
    const uint8_t *offset_bytes = static_cast<const uint8_t *>(offset_rows), *hit_bytes = static_cast<const uint8_t *>(hit_rows);
    auto offset_of = [&](uint32_t r, uint32_t q) {
        uint32_t v;
        std::memcpy(&v, offset_bytes + ((size_t)r * ((size_t)n_queries + 1) + q) * sizeof v, sizeof v);
        return v;
    };
    std::vector<xpbd_overlap_hit> segment;
    uint32_t at = 0;
    for (uint32_t q = 0; q < n_queries; ++q) {
        offsets[q] = at;
        segment.clear();
        uint32_t parts = 0;
        for (uint32_t r = 0; r < n_ranks; ++r) {
            const uint32_t b0 = offset_of(r, q), b1 = offset_of(r, q + 1);
            if (b1 == b0)
                continue;
            ++parts;
            const size_t old = segment.size();
            segment.resize(old + (b1 - b0));
            std::memcpy(segment.data() + old, hit_bytes + ((size_t)r * widest + b0) * sizeof(xpbd_overlap_hit), (size_t)(b1 - b0) * sizeof(xpbd_overlap_hit));
        }
        if (parts > 1)
            std::sort(segment.begin(), segment.end(), [](const xpbd_overlap_hit &a, const xpbd_overlap_hit &b) { return a.body < b.body; });
        for (const xpbd_overlap_hit &h : segment) {
            if (at < cap)
                hits[at] = h;
            ++at;
        }
    }
    offsets[n_queries] = at;
    return at;
}

// ---- contact reports ---------------------------------------------------------------------------------------------------------
// pair_rows: n_ranks rows of `pair_width` xpbd_pair_contact, of which rank r filled pair_counts[r]; first_point indexes the
// rank's row of point_rows (n_ranks rows of `point_width` xpbd_contact_point).  The ranks' lists are disjoint (a pair belongs
// to the owner of its lower body).  pairs = all of them in key order (body_a << 32 | body_b) with first_point re-based into
// `points`, the pairs' points in that order; keys = the keys, ascending.
inline void merge_contact_reports(const void *pair_rows, uint32_t pair_width, const uint32_t *pair_counts, const void *point_rows, uint32_t point_width,
                                  uint32_t n_ranks, std::vector<xpbd_pair_contact> &pairs, std::vector<xpbd_contact_point> &points,
                                  std::vector<uint64_t> &keys)
{
    const uint8_t *pair_bytes = static_cast<const uint8_t *>(pair_rows), *point_bytes = static_cast<const uint8_t *>(point_rows);
    auto pair_at = [&](uint32_t r, uint32_t i) {
        xpbd_pair_contact c;
        std::memcpy(&c, pair_bytes + ((size_t)r * pair_width + i) * sizeof c, sizeof c);
        return c;
    };
    struct Item {
        uint64_t key;
        uint32_t rank, row;
    };
    std::vector<Item> items;
    for (uint32_t r = 0; r < n_ranks; ++r)
        for (uint32_t i = 0; i < pair_counts[r]; ++i) {
            const xpbd_pair_contact c = pair_at(r, i);
            items.push_back(Item{(uint64_t)c.body_a << 32 | c.body_b, r, i});
        }
    std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.key < b.key; });
    pairs.resize(items.size());
    keys.resize(items.size());
    points.clear();
    for (size_t i = 0; i < items.size(); ++i) {
        xpbd_pair_contact c = pair_at(items[i].rank, items[i].row);
        const size_t from = (size_t)items[i].rank * point_width + c.first_point, old = points.size();
        c.first_point = (uint32_t)old;
        points.resize(old + c.n_points);
        if (c.n_points)
            std::memcpy(points.data() + old, point_bytes + from * sizeof(xpbd_contact_point), (size_t)c.n_points * sizeof(xpbd_contact_point));
        pairs[i] = c;
        keys[i] = items[i].key;
    }
}

// The events of a frame from the keys of its touching pairs and of the previous frame's (both ascending): the BEGINs (keys -
// prev) in key order, then the ENDs (prev - keys) in key order.  Returns the number of BEGINs.
inline uint32_t contact_events(const std::vector<uint64_t> &keys, const std::vector<uint64_t> &prev, std::vector<xpbd_contact_event> &events)
{
    std::vector<xpbd_contact_event> ends;
    events.clear();
    size_t a = 0, b = 0;
    while (a < keys.size() || b < prev.size()) {
        if (b == prev.size() || (a < keys.size() && keys[a] < prev[b])) {
            events.push_back(xpbd_contact_event{(uint32_t)(keys[a] >> 32), (uint32_t)keys[a], XPBD_CONTACT_BEGIN});
            ++a;
        } else if (a == keys.size() || prev[b] < keys[a]) {
            ends.push_back(xpbd_contact_event{(uint32_t)(prev[b] >> 32), (uint32_t)prev[b], XPBD_CONTACT_END});
            ++b;
        } else {
            ++a, ++b;
        }
    }
    const uint32_t begins = (uint32_t)events.size();
    events.insert(events.end(), ends.begin(), ends.end());
    return begins;
}

} // namespace xpbd
