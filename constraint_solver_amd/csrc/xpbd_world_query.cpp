// xpbd_world_query.cpp -- scene queries of the single-GPU world (ray casts, overlaps, sweeps, distances): the host layer the multi-GPU
// world shares (xpbd_internal.h) and the entry points.  The argument checks: xpbd_checks.cpp.
#include "xpbd_world.hpp"

namespace xpbd {

// The terrain a query with these flags asks about (null: none; the checks have refused the flag on a world without one).
const Terrain *query_terrain(const xpbd_world *w, uint32_t flags) { return (flags & XPBD_QUERY_TERRAIN) && w->terrain.planes ? &w->terrain : nullptr; }

// The filter table a masked query reads (null: unmasked, or no filters set -- every body is then in group ~0u).
const uint2 *masked_filter(const xpbd_world *w, bool masked) { return masked && w->filters.on ? w->ft_filters.as<uint2>() : nullptr; }

// The host variant of a query with one result per record: n records in, enqueue(device records, device results), n results out,
// and the stream synchronised.
template <class In, class Out, class Enqueue>
int query_host(xpbd_world *w, const In *in, uint32_t n, Out *out, Enqueue &&enqueue)
{
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    SceneQueryScratch &s = w->query;
    const size_t in_bytes = (size_t)n * sizeof(In), out_bytes = (size_t)n * sizeof(Out);
    XPBD_HIP_TRY(s.reserve(QuerySizes{}, in_bytes, out_bytes, 0, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(s.in.ptr, in, in_bytes, hipMemcpyHostToDevice, w->stream));
    if (int rc = enqueue(s.in.as<In>(), s.out.as<Out>()))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(out, s.out.ptr, out_bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

// The prologue of the queries whose records are an overlap query's (overlaps, sweeps, distances): the device bound, room for the
// scratch of n of them over the world's bodies, and the view of it.
static int group_scratch(xpbd_world *w, uint32_t n, bool brute, QueryScratch &scratch)
{
    if (int rc = bind_device(w))
        return rc;
    const QuerySizes q = overlap_scratch_bytes(w->n, n, brute);
    XPBD_HIP_TRY(w->query.reserve(q, 0, 0, 0, w->stream));
    scratch = w->query.view(q.table_size);
    return XPBD_OK;
}

int raycast_enqueue(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *dev_hits,
                    const uint32_t *dev_global_id, bool masked, uint32_t mask)
{
    static_assert(sizeof(xpbd_ray) == 64 && sizeof(xpbd_ray_hit) == 64, "xpbd_ray and xpbd_ray_hit are 64 bytes");
    if (n_rays == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // (a world without bodies takes the brute-force path too: every ray misses, no grid to build)
    const bool brute = (flags & XPBD_RAYCAST_BRUTE_FORCE) || n_rays <= XPBD_RAYCAST_BRUTE_FORCE_RAYS || w->n == 0;
    const QuerySizes q = query_scratch_bytes(w->n, n_rays, brute);
    XPBD_HIP_TRY(w->query.reserve(q, 0, 0, 0, w->stream));
    const RayFilter filter{masked_filter(w, masked), mask, masked ? 1u : 0u};
    XPBD_HIP_TRY(launch_raycast(w->arrays(), w->geom.tables(), dev_global_id, filter, dev_rays, n_rays, brute, w->query.view(q.table_size), dev_hits,
                                w->stream, query_terrain(w, flags), (flags & XPBD_RAYCAST_BRUTE_FORCE) != 0));
    return XPBD_OK;
}

int raycast_host(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits, const uint32_t *dev_global_id,
                 bool masked, uint32_t mask)
{
    return query_host(w, rays, n_rays, hits, [&](const xpbd_ray *dev_rays, xpbd_ray_hit *dev_hits) {
        return raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, dev_global_id, masked, mask);
    });
}

int overlap_enqueue(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags, uint32_t *dev_offsets,
                    xpbd_overlap_hit *dev_hits, uint32_t cap, const uint32_t *dev_global_id)
{
    static_assert(sizeof(xpbd_overlap_query) == 72 && sizeof(xpbd_overlap_hit) == 16, "xpbd_overlap_query is 72 bytes, xpbd_overlap_hit 16");
    if (n_queries == 0) {
        if (int rc = bind_device(w))
            return rc;
        if (dev_offsets)
            XPBD_HIP_TRY(hipMemsetAsync(dev_offsets, 0, sizeof(uint32_t), w->stream));
        return XPBD_OK;
    }
    const bool brute = (flags & XPBD_OVERLAP_BRUTE_FORCE) || w->n == 0;
    QueryScratch scratch;
    XPBD_TRY(group_scratch(w, n_queries, brute, scratch));
    const bool masked = (flags & XPBD_OVERLAP_MASKED) != 0;
    XPBD_HIP_TRY(launch_overlap(w->arrays(), w->geom.tables(), dev_global_id, masked_filter(w, masked), dev_queries, n_queries, masked, brute, scratch,
                                dev_offsets, dev_hits, cap, w->stream, query_terrain(w, flags)));
    return XPBD_OK;
}

int overlap_host(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets, xpbd_overlap_hit *hits,
                 uint32_t cap, uint32_t *n_out, const uint32_t *dev_global_id)
{
    *n_out = 0;
    if (n_queries == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    SceneQueryScratch &s = w->query;
    const size_t q_bytes = (size_t)n_queries * sizeof(xpbd_overlap_query), o_bytes = ((size_t)n_queries + 1) * sizeof(uint32_t);
    XPBD_HIP_TRY(s.reserve(QuerySizes{}, q_bytes, (size_t)at_least_one(cap) * sizeof(xpbd_overlap_hit), o_bytes, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(s.in.ptr, queries, q_bytes, hipMemcpyHostToDevice, w->stream));
    if (int rc = overlap_enqueue(w, s.in.as<xpbd_overlap_query>(), n_queries, flags, s.offsets.as<uint32_t>(),
                                 cap ? s.out.as<xpbd_overlap_hit>() : nullptr, cap, dev_global_id))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(offsets, s.offsets.ptr, o_bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = offsets[n_queries], held = total < cap ? total : cap;
    if (held) {
        XPBD_HIP_TRY(hipMemcpyAsync(hits, s.out.ptr, (size_t)held * sizeof(xpbd_overlap_hit), hipMemcpyDeviceToHost, w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    *n_out = total;
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "overlap query: %u hits but room for %u", total, cap);
    return XPBD_OK;
}

int sweep_enqueue(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *dev_hits,
                  const uint32_t *dev_global_id)
{
    static_assert(sizeof(xpbd_sweep) == 104 && sizeof(xpbd_sweep_hit) == 72, "xpbd_sweep is 104 bytes, xpbd_sweep_hit 72");
    if (n_sweeps == 0)
        return XPBD_OK;
    // (a shard without bodies takes the brute-force path too: every sweep misses, no grid to build)
    const bool brute = (flags & XPBD_SWEEP_BRUTE_FORCE) || n_sweeps <= XPBD_SWEEP_BRUTE_FORCE_SWEEPS || w->n == 0;
    QueryScratch scratch;
    XPBD_TRY(group_scratch(w, n_sweeps, brute, scratch));
    const bool masked = (flags & XPBD_SWEEP_MASKED) != 0;
    XPBD_HIP_TRY(launch_sweep(w->arrays(), w->geom.tables(), dev_global_id, masked_filter(w, masked), dev_sweeps, n_sweeps, masked, brute, scratch,
                              dev_hits, w->stream, query_terrain(w, flags), (flags & XPBD_SWEEP_BRUTE_FORCE) != 0));
    return XPBD_OK;
}

int sweep_host(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits, const uint32_t *dev_global_id)
{
    return query_host(w, sweeps, n_sweeps, hits, [&](const xpbd_sweep *dev_sweeps, xpbd_sweep_hit *dev_hits) {
        return sweep_enqueue(w, dev_sweeps, n_sweeps, flags, dev_hits, dev_global_id);
    });
}

int distance_enqueue(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *dev_hits,
                     const uint32_t *dev_global_id)
{
    static_assert(sizeof(xpbd_distance_query) == 80 && sizeof(xpbd_distance_hit) == 96, "xpbd_distance_query is 80 bytes, xpbd_distance_hit 96");
    if (n_queries == 0)
        return XPBD_OK;
    // (a shard without bodies takes the brute-force path too: every query finds nothing, no grid to build)
    const bool brute = (flags & XPBD_DISTANCE_BRUTE_FORCE) || n_queries <= XPBD_DISTANCE_BRUTE_FORCE_QUERIES || w->n == 0;
    QueryScratch scratch;
    XPBD_TRY(group_scratch(w, n_queries, brute, scratch));
    const bool masked = (flags & XPBD_DISTANCE_MASKED) != 0;
    XPBD_HIP_TRY(launch_distance(w->arrays(), w->geom.tables(), dev_global_id, masked_filter(w, masked), dev_queries, n_queries, masked, brute, scratch,
                                 dev_hits, w->stream));
    return XPBD_OK;
}

int distance_host(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits,
                  const uint32_t *dev_global_id)
{
    return query_host(w, queries, n_queries, hits, [&](const xpbd_distance_query *dev_queries, xpbd_distance_hit *dev_hits) {
        return distance_enqueue(w, dev_queries, n_queries, flags, dev_hits, dev_global_id);
    });
}

int terrain_distance_enqueue(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *dev_hits)
{
    if (n_queries == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // (without polytopes the shape table is empty: every shape index is outside it, and only the point volume finds anything)
    const PolytopeTables tables = w->geom.has_topology ? w->geom.tables() : PolytopeTables{};
    XPBD_HIP_TRY(launch_terrain_distance(TerrainHeights{w->terrain, w->tr_heights.as<double>()}, tables, dev_queries, n_queries,
                                         (flags & XPBD_DISTANCE_BRUTE_FORCE) != 0, dev_hits, w->stream));
    return XPBD_OK;
}

int terrain_distance_host(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits)
{
    return query_host(w, queries, n_queries, hits, [&](const xpbd_distance_query *dev_queries, xpbd_distance_hit *dev_hits) {
        return terrain_distance_enqueue(w, dev_queries, n_queries, flags, dev_hits);
    });
}

} // namespace xpbd

extern "C" {

namespace { // (inside the extern "C" block, where it has always been: it keeps its unmangled name in the library)
// What the scene queries' argument checks (xpbd_checks.hpp) need to know of world `w`, for the entry point `who`: XPBD_OK and
// *target, or the error of a NULL world.
int query_target(const char *who, const xpbd_world *w, xpbd::QueryTarget *target)
{
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    *target = {w->geom.has_topology, w->n, w->geom.n_shapes, "xpbd_world_set_polytopes (set_shapes gives vertices only)", true, w->terrain.planes != nullptr};
    return XPBD_OK;
}
} // namespace

int xpbd_world_raycast(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits)
try {
    const char *who = "xpbd_world_raycast";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_raycast(who, target, rays, n_rays, flags, hits, true));
    return xpbd::raycast_host(w, rays, n_rays, flags, hits, nullptr, false, 0u);
} XPBD_ABI_CATCH

int xpbd_world_raycast_masked(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, uint32_t mask, xpbd_ray_hit *hits)
try {
    const char *who = "xpbd_world_raycast_masked";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_raycast(who, target, rays, n_rays, flags, hits, true));
    return xpbd::raycast_host(w, rays, n_rays, flags, hits, nullptr, true, mask);
} XPBD_ABI_CATCH

int xpbd_world_raycast_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *dev_hits)
try {
    const char *who = "xpbd_world_raycast_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_raycast(who, target, dev_rays, n_rays, flags, dev_hits, false));
    return xpbd::raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, nullptr, false, 0u);
} XPBD_ABI_CATCH

int xpbd_world_raycast_masked_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, uint32_t mask,
                                     xpbd_ray_hit *dev_hits)
try {
    const char *who = "xpbd_world_raycast_masked_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_raycast(who, target, dev_rays, n_rays, flags, dev_hits, false));
    return xpbd::raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, nullptr, true, mask);
} XPBD_ABI_CATCH

int xpbd_world_overlap(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                       xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
try {
    const char *who = "xpbd_world_overlap";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_overlap(who, target, queries, n_queries, flags, offsets, hits, cap, n_out, true));
    uint32_t total = 0;
    const int rc = xpbd::overlap_host(w, queries, n_queries, flags, offsets, hits, cap, &total, nullptr);
    if (n_out && (rc == XPBD_OK || rc == XPBD_E_CAPACITY))
        *n_out = total;
    return rc;
} XPBD_ABI_CATCH

int xpbd_world_overlap_device(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags, uint32_t *dev_offsets,
                              xpbd_overlap_hit *dev_hits, uint32_t cap)
try {
    const char *who = "xpbd_world_overlap_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_overlap(who, target, dev_queries, n_queries, flags, dev_offsets, dev_hits, cap, nullptr, false));
    return xpbd::overlap_enqueue(w, dev_queries, n_queries, flags, dev_offsets, dev_hits, cap, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_sweep(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
try {
    const char *who = "xpbd_world_sweep";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_sweep(who, target, sweeps, n_sweeps, flags, hits, true));
    return xpbd::sweep_host(w, sweeps, n_sweeps, flags, hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_sweep_device(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *dev_hits)
try {
    const char *who = "xpbd_world_sweep_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_sweep(who, target, dev_sweeps, n_sweeps, flags, dev_hits, false));
    return xpbd::sweep_enqueue(w, dev_sweeps, n_sweeps, flags, dev_hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_distance(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits)
try {
    const char *who = "xpbd_world_distance";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_distance(who, target, queries, n_queries, flags, hits, true));
    return xpbd::distance_host(w, queries, n_queries, flags, hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_distance_device(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *dev_hits)
try {
    const char *who = "xpbd_world_distance_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_distance(who, target, dev_queries, n_queries, flags, dev_hits, false));
    return xpbd::distance_enqueue(w, dev_queries, n_queries, flags, dev_hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_terrain_distance(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits)
try {
    const char *who = "xpbd_world_terrain_distance";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_terrain_distance(who, target, queries, n_queries, flags, hits, true));
    return xpbd::terrain_distance_host(w, queries, n_queries, flags, hits);
} XPBD_ABI_CATCH

int xpbd_world_terrain_distance_device(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags,
                                       xpbd_distance_hit *dev_hits)
try {
    const char *who = "xpbd_world_terrain_distance_device";
    xpbd::QueryTarget target;
    XPBD_TRY(query_target(who, w, &target));
    XPBD_TRY(xpbd::check_terrain_distance(who, target, dev_queries, n_queries, flags, dev_hits, false));
    return xpbd::terrain_distance_enqueue(w, dev_queries, n_queries, flags, dev_hits);
} XPBD_ABI_CATCH

} // extern "C"
