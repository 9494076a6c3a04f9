// xpbd_query.h -- scene queries (EXTENSION): launchers for the batched ray casts, overlap queries, sweep queries and distance queries.
// One unit per family -- xpbd_query_rays.hip, xpbd_query_overlap.hip, xpbd_query_sweep.hip, xpbd_query_distance.hip -- on top of
// xpbd_query_grid.hip (the bodies' records, the grid, the scratch); the device routines more than one family uses are in
// xpbd_query_device.hpp, which opens with the table of who uses what.  The terrain's passes: xpbd_terrain_query.hip.
//
// Semantics: include/xpbd.h, "Scene queries".  Two paths give the same bits in every field of every hit:
//  * grid: the bodies' bounding spheres (frame * centroid, PolytopeTables::radii) go into a uniform grid built for this call
//    (cell edge just above 2 x the largest radius, so a sphere overlaps at most 2 x 2 x 2 cells; dense linear keys when the
//    box of all spheres fits the table, hashed keys otherwise), and every ray walks its cells in order (3D-DDA), testing the
//    bodies listed there, until the next cell starts beyond the best hit;
//  * brute force: every ray against every body, reduced on (t, index) across lanes, waves and workgroups.
// Both use one routine for a (ray, body) pair (ray_body in xpbd_query_shared.hpp) and the same total order on candidates, so the
// winner -- the minimum -- does not depend on which bodies were tested how often or in which order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime_api.h>

#include "xpbd_internal.h"
#include "xpbd_kernels.h"
#include "xpbd_pairs.h"

namespace xpbd {

// Per body, written by the first pass of every call: inverse frame (position xyz, rotation s x y z), sphere centre xyz and
// radius (radius < 0: the body is never hit -- its pose is not finite, or it is a ghost of a multi-GPU shard).
constexpr uint32_t kQueryRecDoubles = 12;

// Device scratch of one call (a view of SceneQueryScratch, which owns it).
struct QueryScratch {
    double *rec;          // [n][kQueryRecDoubles]
    double *partials;     // [blocks_for(n)][7]
    void *grid;           // one QueryGrid (xpbd_query_device.hpp)
    uint32_t *cell_start; // [table_size + 1]: exclusive scan of the cell populations
    uint32_t *cell_fill;  // [table_size]
    uint32_t *items;      // [8 n]: body slots, grouped by cell
    uint32_t *scan_scratch;
    void *brute;          // per (ray, workgroup of bodies) partial winners of the brute-force ray cast
    double *qrec;         // per overlap query: sphere centre, radius
    uint32_t table_size;  // power of two
};

struct QuerySizes {
    size_t rec, partials, grid, cell_start, cell_fill, items, scan_scratch, brute, qrec;
    uint32_t table_size;
};
// What a ray cast over n bodies and n_rays rays needs (brute: whether it takes the brute-force path).
QuerySizes query_scratch_bytes(uint32_t n, uint32_t n_rays, bool brute);

// The scene queries' device memory of one world: the scratch of a call, shared by the ray casts, the overlap, the sweep and the
// distance queries, and the staging of the host variants' arrays (rays or queries in, hits out, an overlap's offsets).  One call uses it at a time:
// the calls of a world are ordered on its stream, and every host variant ends with a wait.
struct SceneQueryScratch {
    DeviceBuffer rec, partials, grid, cell_start, cell_fill, items, scan, brute, qrec;
    DeviceBuffer in, out, offsets;

    // Room for a call's scratch and staging (sizes of 0: not needed); waits for `stream` only if something has to grow.
    hipError_t reserve(const QuerySizes &q, size_t in_bytes, size_t out_bytes, size_t offsets_bytes, hipStream_t stream) noexcept;
    QueryScratch view(uint32_t table_size) const;
};

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
// terrain (null: no terrain pass): after the body pass, on the same stream, launch_terrain_rays puts the terrain's answer next to
// the bodies' (XPBD_QUERY_TERRAIN); terrain_brute: every ray against every triangle instead of the walk.
hipError_t launch_raycast(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const RayFilter &filter, const void *rays,
                          uint32_t n_rays, bool brute, const QueryScratch &s, void *hits, hipStream_t stream, const Terrain *terrain = nullptr,
                          bool terrain_brute = false);

// ---- overlap queries: which bodies does each convex volume touch? (include/xpbd.h, "Overlap queries") ---------------------
// Passes: the bounding spheres of the bodies (k_query_bodies) and of the queries (k_overlap_queries); on the grid path the grid
// of a ray cast (k_query_grid, k_query_bin); a COUNT pass -- one group of 16 / 32 / 64 lanes per query tests its candidates
// (ignore_body and mask, tight spheres, the decision part of the SAT) and leaves one number per query; an exclusive scan of
// the numbers, which is the caller's `offsets`; a FILL pass that repeats the tests and writes the hits; a sort of every
// query's segment into ascending body index.  Testing twice avoids any list whose length only the host could learn, so the
// whole call is stream-ordered.  The brute-force path visits the bodies of every query in ascending index instead of walking
// cells (no grid, no sort); a segment that the caller's `cap` cuts short is listed that way on the grid path too.
constexpr uint32_t kOverlapSortStage = 1024; // hits of one query sorted in LDS; longer segments are sorted in global memory

// The scratch shared with the ray casts (scan_scratch also covers the scan of the offsets; no brute-force partials) and qrec.
QuerySizes overlap_scratch_bytes(uint32_t n, uint32_t n_queries, bool brute);

// n_queries device xpbd_overlap_query against the bodies of `b`: offsets[n_queries + 1] (device) receives the CSR offsets of
// the full answer, hits[0 .. min(total, cap)) (device xpbd_overlap_hit; may be null with cap == 0) its first entries.
// global_id as for launch_raycast; filter: the bodies' collision filters (null: every body in group ~0u), tested against the
// queries' masks when `masked`.
hipError_t launch_overlap(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries,
                          uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, uint32_t *offsets, void *hits, uint32_t cap,
                          hipStream_t stream, const Terrain *terrain = nullptr);

// ---- sweep queries: the first body a translating convex volume hits (include/xpbd.h, "Sweep queries") ----------------------
// Passes: the bounding spheres of the bodies (k_query_bodies) and of the volumes at t = 0 (k_sweep_queries, the records of an
// overlap query); on the grid path the grid of a ray cast; then one group of 16 / 32 / 64 lanes per sweep walks the cells of
// its centre line as a ray does, looks for every stretch of it at the bodies in the cells the volume's sphere covers, and keeps
// the minimum under (t, index).  The brute-force path visits every body instead.  A sweep's scratch is an overlap's
// (overlap_scratch_bytes with the number of sweeps).
hipError_t launch_sweep(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *sweeps,
                        uint32_t n_sweeps, bool masked, bool brute, const QueryScratch &s, void *hits, hipStream_t stream,
                        const Terrain *terrain = nullptr, bool terrain_brute = false);

// ---- distance queries: the body nearest to a convex volume or a point (include/xpbd.h, "Distance queries") ----------------
// Passes: the bounding spheres of the bodies (k_query_bodies) and of the volumes (k_distance_queries, the records of an overlap
// query); on the grid path the grid of a ray cast; then one group of 16 / 32 / 64 lanes per query walks the cells the volume's
// sphere covers and then those the sphere grown by min(max_distance, best so far) covers, decides every candidate -- the overlap
// query's decision, the vertex-face candidates, the edge pairs -- and keeps the minimum under (distance, index).  The brute-force
// path, and a query that reaches further than kSweepReach cell edges, visits every body instead.  A distance query's scratch is
// an overlap's (overlap_scratch_bytes with the number of queries).  No terrain: launch_terrain_distance below is a call of its own.
hipError_t launch_distance(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries,
                           uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, void *hits, hipStream_t stream);

// ---- the terrain in the scene queries (include/xpbd.h, "Terrain in the scene queries"; xpbd_terrain_query.hip) ---------------
// Each is one kernel on `stream`, called by the three launchers above when they are given a terrain, and reads the plane table of
// k_terrain_planes alone.
//  * rays: after the body pass.  One lane per ray reads hits[r], walks the cells under the ray's xy-projection (a 2D DDA whose
//    border times come from the slab expression of each border; `brute`: every triangle instead) no further than that distance,
//    and overwrites the record only if the terrain wins under (t, body).
//  * sweeps: after k_sweep_pass.  32 lanes per sweep, one per vertex of the volume, each casting its vertex as a ray no further
//    than hits[q].distance; the minimum under (t, triangle, vertex) replaces the record only if it is strictly earlier.
//    qrec: k_sweep_queries' records (radius < 0: the sweep hits nothing).
//  * overlaps: one lane per query looks every vertex up as the stepper does.  fill == false, between the count pass and the
//    scan: offsets[q] += 1 for a volume with a vertex under the ground; fill == true, after the fill pass and before the sort:
//    its entry at offsets[q + 1] - 1 when that slot is below cap.  qrec: k_overlap_queries' records.
hipError_t launch_terrain_rays(const Terrain &terrain, const void *rays, uint32_t n_rays, bool brute, void *hits, hipStream_t stream);
hipError_t launch_terrain_sweeps(const Terrain &terrain, const PolytopeTables &t, const void *sweeps, uint32_t n_sweeps, bool brute, const double *qrec,
                                 void *hits, hipStream_t stream);
hipError_t launch_terrain_overlap(const Terrain &terrain, const PolytopeTables &t, const void *queries, uint32_t n_queries, bool fill, const double *qrec,
                                  uint32_t *offsets, void *hits, uint32_t cap, hipStream_t stream);

// ---- the terrain in the distance queries (include/xpbd.h, "Terrain in the distance queries"; xpbd_terrain_query.hip) -----------
// A call of its own (xpbd_world_terrain_distance), not a pass after launch_distance.  What the kernel reads of the field: the
// stepper's Terrain, unchanged (its kernels take it by value), and the heights the plane table was made from, ny rows of nx.
struct TerrainHeights {
    Terrain tr;
    const double *heights;
};
// One kernel on `stream`: a group of 8 lanes per query walks rings of samples around the one under the volume's centre
// (`brute`: every sample), each lane deciding what its sample owns -- two triangles, the sample, up to three edges -- and the
// group keeps the minimum under (d2, class, terrain feature, volume index).  It writes hits[0 .. n_queries) and nothing else: no
// atomics, no scratch of its own, so the device variant never waits.  `t` may be an empty table (n_shapes == 0): only point
// queries then find anything.
hipError_t launch_terrain_distance(const TerrainHeights &terrain, const PolytopeTables &t, const void *queries, uint32_t n_queries, bool brute, void *hits,
                                   hipStream_t stream);

} // namespace xpbd
