// xpbd_checks_terrain_distance.hpp -- the argument check of the terrain distance queries (include/xpbd.h, "Terrain in the distance
// queries"), defined in xpbd_checks.cpp beside check_distance and host-only like it.  A header of its own for the reason
// xpbd_checks_distance.hpp is one: the tests hold each of the older headers to the set of checks it declared.
#pragma once

#include "xpbd_checks.hpp"

namespace xpbd {

// NULL arrays, unknown flags (everything but XPBD_DISTANCE_BRUTE_FORCE and XPBD_DISTANCE_MASKED, XPBD_QUERY_TERRAIN included),
// with `host` a nonzero `reserved`, a target without a terrain.  Neither polytopes nor bodies are required: without polytopes
// only point queries find anything.
int check_terrain_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                           const void *hits, bool host);

} // namespace xpbd
