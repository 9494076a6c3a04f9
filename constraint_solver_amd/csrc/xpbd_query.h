// xpbd_query.h -- scene queries (EXTENSION): launchers for the batched ray casts in xpbd_query.hip.
//
// Semantics: include/xpbd.h, "Scene queries".  Two paths give the same bits in every field of every hit:
//  * grid: the bodies' bounding spheres (frame * centroid, PolytopeTables::radii) go into a uniform grid built for this call
//    (cell edge just above 2 x the largest radius, so a sphere overlaps at most 2 x 2 x 2 cells; dense linear keys when the
//    box of all spheres fits the table, hashed keys otherwise), and every ray walks its cells in order (3D-DDA), testing the
//    bodies listed there, until the next cell starts beyond the best hit;
//  * brute force: every ray against every body, reduced on (t, index) across lanes, waves and workgroups.
// Both use one routine for a (ray, body) pair (ray_body in xpbd_query.hip) and the same total order on candidates, so the
// winner -- the minimum -- does not depend on which bodies were tested how often or in which order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime_api.h>

#include "xpbd_kernels.h"
#include "xpbd_pairs.h"

namespace xpbd {

// Per body, written by the first pass of every call: inverse frame (position xyz, rotation s x y z), sphere centre xyz and
// radius (radius < 0: the body is never hit -- its pose is not finite, or it is a ghost of a multi-GPU shard).
constexpr uint32_t kQueryRecDoubles = 12;

// Device scratch of one call (the owner sizes it with query_scratch_bytes and keeps it).
struct QueryScratch {
    double *rec;          // [n][kQueryRecDoubles]
    double *partials;     // [blocks_for(n)][7]
    void *grid;           // one QueryGrid (xpbd_query.hip)
    uint32_t *cell_start; // [table_size + 1]: exclusive scan of the cell populations
    uint32_t *cell_fill;  // [table_size]
    uint32_t *items;      // [8 n]: body slots, grouped by cell
    uint32_t *scan_scratch;
    void *brute;          // per (ray, workgroup of bodies) partial winners of the brute-force path
    uint32_t table_size;  // power of two
};

struct QuerySizes {
    size_t rec, partials, grid, cell_start, cell_fill, items, scan_scratch, brute;
    uint32_t table_size;
};
// What a call over n bodies and n_rays rays needs (brute: whether it takes the brute-force path).
QuerySizes query_scratch_bytes(uint32_t n, uint32_t n_rays, bool brute);

// The collision-filter test of a masked ray cast: with `masked`, body i answers only if (group_i & mask) != 0, group_i =
// filter[i].x (filter == NULL: every body is in group ~0u).  Without it no group is tested.
struct RayFilter {
    const uint2 *filter;
    uint32_t mask;
    uint32_t masked;
};

// Casts n_rays rays (device xpbd_ray) against the bodies of `b` and writes n_rays xpbd_ray_hit.  global_id (device, n entries,
// or null): the index a body is known by -- the tie-break and what ignore_body and hit.body mean -- and XPBD_NO_HIT for a
// body that must not answer; null: the body's slot.  A body the filter drops answers no ray, as a ghost does.
hipError_t launch_raycast(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const RayFilter &filter, const void *rays,
                          uint32_t n_rays, bool brute, const QueryScratch &s, void *hits, hipStream_t stream);

} // namespace xpbd
