// islands_checks_standalone_main.cpp -- IslandsTarget::check (csrc/xpbd_checks.cpp, declared in csrc/xpbd_checks.hpp), the
// argument check of xpbd_world_islands and xpbd_world_islands_device, built with plain g++ (no hipcc, no ROCm include path; see
// test_islands_checks_standalone.py): every way it refuses a call, each with XPBD_E_INVALID and a message that names the `who`
// it was given, and the calls it accepts.  Exits 0.
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
    const IslandsTarget reported{4, true, true}, no_frame{4, true, false}, off{4, false, false}, empty{0, true, true};
    xpbd_island records[2] = {};
    uint32_t count = 0;

    accepted(reported.check("ok_all_edges", 0, records, 2, &count), "both kinds of edges with a report frame");
    accepted(reported.check("ok_no_joints", XPBD_ISLANDS_NO_JOINTS, records, 2, &count), "contacts only");
    accepted(off.check("ok_joints_only", XPBD_ISLANDS_NO_CONTACTS, records, 2, &count), "joints only needs no report");
    accepted(no_frame.check("ok_count_only", XPBD_ISLANDS_NO_CONTACTS, nullptr, 0, &count), "no records with cap 0");
    refused(reported.check("null_count", 0, records, 2, nullptr), "null_count", "NULL count");
    refused(reported.check("null_records", 0, nullptr, 2, &count), "null_records", "NULL records");
    refused(reported.check("flag_4", 4u, records, 2, &count), "flag_4", "unknown flags");
    refused(reported.check("flag_high", 0x80000000u | XPBD_ISLANDS_NO_JOINTS, records, 2, &count), "flag_high", "unknown flags");
    refused(reported.check("both_flags", XPBD_ISLANDS_NO_JOINTS | XPBD_ISLANDS_NO_CONTACTS, records, 2, &count), "both_flags", "together");
    refused(empty.check("no_bodies", XPBD_ISLANDS_NO_CONTACTS, records, 2, &count), "no_bodies", "no bodies");
    refused(off.check("reports_off", 0, records, 2, &count), "reports_off", "reports are off");
    refused(off.check("reports_off_no_joints", XPBD_ISLANDS_NO_JOINTS, records, 2, &count), "reports_off_no_joints", "reports are off");
    refused(no_frame.check("no_frame", 0, records, 2, &count), "no_frame", "no report");

    if (failures)
        return 1;
    std::printf("%d calls ok\n", calls);
    return 0;
}
