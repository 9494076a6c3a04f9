// xpbd_query_units.hpp -- scene queries (EXTENSION): what the query units (xpbd_query_grid.hip, _rays.hip, _overlap.hip,
// _sweep.hip, _distance.hip) share on the host side, on top of the device routines of xpbd_query_device.hpp.  Not installed.
#pragma once

#include <type_traits>

#include "xpbd_query_device.hpp"

namespace xpbd {

// xpbd_query_grid.hip: the passes every family begins with.
// The first pass of every call: the bodies' records and the partial bounds of their spheres.
void launch_query_bodies(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const RayFilter &filter, const QueryScratch &s,
                         hipStream_t stream);
// The grid over the bodies' spheres: its dimensions, the cells' populations, their scan, the bodies grouped by cell.
hipError_t launch_query_grid(const BodyArrays &b, const QueryScratch &s, hipStream_t stream);

namespace {

inline uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

inline uint32_t brute_chunks(uint32_t n, uint32_t n_rays)
{
    const uint32_t tiles = (n_rays + kBruteRays - 1) / kBruteRays;
    uint32_t chunks = (kBruteBlocks + tiles - 1) / (tiles ? tiles : 1);
    const uint32_t most = blocks_of(n) ? blocks_of(n) : 1; // at least one body block (kBlock bodies) per workgroup
    return chunks < 1 ? 1 : (chunks > most ? most : chunks);
}

inline PassArgs pass_args(const QueryScratch &s, const uint32_t *global_id, const uint2 *filter, uint32_t n, bool masked, bool brute)
{
    return PassArgs{s.qrec, s.rec, global_id, filter, static_cast<QueryGrid *>(s.grid), s.cell_start, s.items, n, masked ? 1u : 0u, brute ? 1u : 0u};
}

// Lanes per query (L) and vertex capacity (V) of the group kernels by the largest shape, as the SAT launchers of the contact
// pipeline choose theirs: launch(L, V, workgroups) with L and V as std::integral_constant, 64 / L queries per workgroup.
template <class Launch>
void with_group_shape(const PolytopeTables &t, uint32_t n_queries, Launch &&launch)
{
    using std::integral_constant;
    if (t.max_verts <= 8 && t.max_faces <= 8)
        launch(integral_constant<uint32_t, 16>{}, integral_constant<uint32_t, 8>{}, dim3((n_queries + 3) / 4));
    else if (t.max_verts <= 16)
        launch(integral_constant<uint32_t, 32>{}, integral_constant<uint32_t, 16>{}, dim3((n_queries + 1) / 2));
    else
        launch(integral_constant<uint32_t, 64>{}, integral_constant<uint32_t, XPBD_MAX_SHAPE_VERTS>{}, dim3(n_queries));
}

} // namespace

} // namespace xpbd
