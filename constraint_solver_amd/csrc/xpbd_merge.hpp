// xpbd_merge.hpp -- how the multi-GPU world (xpbd_multi.cpp) merges the scene queries' answers of its ranks.  Host-only: pure
// functions of the gathered bytes, no device and no collective (tests/merge_standalone_main.cpp runs them on their own).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/xpbd.h"

namespace xpbd {

// rows: n_ranks rows of n_rays xpbd_ray_hit, rank r's answer for its owned bodies (a miss: XPBD_NO_HIT at +inf).  out[i] = the
// minimum over the ranks under the order of a single world: distance, then body.
inline void merge_ray_hits(const void *rows, uint32_t n_ranks, uint32_t n_rays, xpbd_ray_hit *out)
{
    const uint8_t *bytes = static_cast<const uint8_t *>(rows);
    for (uint32_t i = 0; i < n_rays; ++i) {
        xpbd_ray_hit best;
        std::memcpy(&best, bytes + (size_t)i * sizeof best, sizeof best);
        for (uint32_t r = 1; r < n_ranks; ++r) {
            xpbd_ray_hit h;
            std::memcpy(&h, bytes + ((size_t)r * n_rays + i) * sizeof h, sizeof h);
            if (h.distance < best.distance || (h.distance == best.distance && h.body < best.body))
                best = h;
        }
        out[i] = best;
    }
}

// The same for sweeps: rows of n_sweeps xpbd_sweep_hit, the minimum on (distance, body).
inline void merge_sweep_hits(const void *rows, uint32_t n_ranks, uint32_t n_sweeps, xpbd_sweep_hit *out)
{
    const uint8_t *bytes = static_cast<const uint8_t *>(rows);
    for (uint32_t i = 0; i < n_sweeps; ++i) {
        xpbd_sweep_hit best;
        std::memcpy(&best, bytes + (size_t)i * sizeof best, sizeof best);
        for (uint32_t r = 1; r < n_ranks; ++r) {
            xpbd_sweep_hit h;
            std::memcpy(&h, bytes + ((size_t)r * n_sweeps + i) * sizeof h, sizeof h);
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

} // namespace xpbd
