// distance_checks_standalone_main.cpp -- check_distance (csrc/xpbd_checks.cpp, declared in csrc/xpbd_checks.hpp) built with
// plain g++ (no hipcc, no ROCm include path; see test_distance_checks_standalone.py): every way it refuses a call, each with
// XPBD_E_INVALID and a message that names the `who` it was given, and the calls it accepts.  Exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../constraint_solver_amd/csrc/xpbd_checks.hpp"

namespace {

int failures = 0, calls = 0;

void accepted(int rc, const char *what)
{
    ++calls;
    if (rc != XPBD_OK) {
        ++failures;
        std::printf("%s: accepted call returned %d (%s)\n", what, rc, xpbd_last_error());
    }
}

void refused(int rc, const char *who, const char *word)
{
    ++calls;
    if (rc != XPBD_E_INVALID || !std::strstr(xpbd_last_error(), who) || !std::strstr(xpbd_last_error(), word)) {
        ++failures;
        std::printf("%s: refused call returned %d with message '%s' (expected '%s' in it)\n", who, rc, xpbd_last_error(), word);
    }
}

} // namespace

int main()
{
    using namespace xpbd;
    const QueryTarget world{true, 4, 2, "the_setter", true, true}, bare{false, 4, 2, "the_setter", false, false},
        empty{true, 0, 2, "the_setter", false, false};
    xpbd_distance_query q[2] = {};
    xpbd_distance_hit hits[2] = {};
    q[0].shape = XPBD_DISTANCE_POINT;
    q[1].shape = 7; // outside the table of 2 shapes: no error, the query finds nothing

    accepted(check_distance("ok_all_flags", world, q, 2, XPBD_DISTANCE_BRUTE_FORCE | XPBD_DISTANCE_MASKED, hits, true), "every known flag");
    accepted(check_distance("ok_none", world, nullptr, 0, 0, nullptr, true), "n_queries = 0");
    refused(check_distance("null_queries", world, nullptr, 2, 0, hits, true), "null_queries", "NULL");
    refused(check_distance("null_hits", world, q, 2, 0, nullptr, false), "null_hits", "NULL");
    refused(check_distance("flag_4", world, q, 2, 4u, hits, true), "flag_4", "unknown flags");
    // the terrain is no body: its flag is unknown here even for a world that has a terrain and allows the flag elsewhere
    refused(check_distance("flag_terrain", world, q, 2, XPBD_QUERY_TERRAIN | XPBD_DISTANCE_MASKED, hits, true), "flag_terrain", "unknown flags");
    refused(check_distance("no_polytopes", bare, q, 2, 0, hits, true), "no_polytopes", "the_setter");
    refused(check_distance("no_bodies", empty, q, 2, 0, hits, true), "no_bodies", "no bodies");
    q[1].reserved = 3;
    refused(check_distance("reserved", world, q, 2, 0, hits, true), "reserved", "query 1");
    accepted(check_distance("device_variant", world, q, 2, 0, hits, false), "the device variant does not read the records");

    if (failures)
        return 1;
    std::printf("%d calls ok\n", calls);
    return 0;
}
