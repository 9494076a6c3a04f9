// xpbd_checks_distance.hpp -- the argument check of the distance queries (include/xpbd.h, "Distance queries"), defined in
// xpbd_checks.cpp beside the other scene queries' checks and host-only like them.  Declared here and not in xpbd_checks.hpp:
// tests/test_checks_standalone.py holds the set of checks declared there, and its stand-alone program, as they were;
// tests/test_distance_checks_standalone.py runs this one the same way.
#pragma once

#include "xpbd_checks.hpp"

namespace xpbd {

// As check_sweep: NULL arrays, unknown flags, no polytopes, with `host` a nonzero `reserved`, a target without bodies.  A shape
// outside the table (XPBD_DISTANCE_POINT aside) is no error, the query finds nothing; XPBD_QUERY_TERRAIN is an unknown flag whatever
// the target (the terrain is no body).
int check_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, const void *hits,
                   bool host);

} // namespace xpbd
