// sensor_checks_standalone_main.cpp -- SensorTarget::table_check and ::overlaps_check (csrc/xpbd_checks.cpp, declared in
// csrc/xpbd_checks.hpp), the argument checks of xpbd_world_set_sensors / _get_sensors and of xpbd_world_sensor_overlaps and its
// device variant, built with plain g++ (no hipcc, no ROCm include path; see test_sensor_checks_standalone.py): every way they
// refuse a call, each with XPBD_E_INVALID and a message that names the `who` it was given and the reason, and the calls they
// accept.  Exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

void expect(bool ok, const char *what)
{
    ++calls;
    if (!ok) {
        ++failures;
        std::printf("%s\n", what);
    }
}

} // namespace

int main()
{
    using namespace xpbd;
    const SensorTarget ready{4, 2, true, true}, no_frame{4, 2, true, false}, off{4, 2, false, false}, none{4, 0, true, true}, empty{0, 0, true, true};
    const uint8_t flags[4] = {0, 1, 1, 0}, zeros[4] = {0, 0, 0, 0}, two[4] = {0, 2, 0, 0}, high[4] = {0, 0, 0, 0x81};
    uint8_t out[4] = {9, 9, 9, 9};
    uint32_t count = 77;

    // ---- the table: the setter ...
    accepted(ready.table_check("ok_table", flags, 4, false, &count), "a table of the body count");
    expect(count == 2, "ok_table: two bytes are 1");
    accepted(ready.table_check("ok_zeros", zeros, 4, false, &count), "an all-zero table");
    expect(count == 0, "ok_zeros: no byte is 1");
    accepted(ready.table_check("ok_clear", nullptr, 0, false, &count), "NULL with n == 0 clears");
    expect(count == 0, "ok_clear: nothing flagged");
    accepted(empty.table_check("ok_empty_world", nullptr, 0, false), "a world without bodies");
    accepted(ready.table_check("ok_no_count", flags, 4, false), "the count is optional");
    refused(ready.table_check("null_table", nullptr, 4, false), "null_table", "NULL is_sensor");
    refused(ready.table_check("short_table", flags, 3, false), "short_table", "holds 4 bodies");
    refused(ready.table_check("long_table", flags, 5, false), "long_table", "holds 4 bodies");
    refused(ready.table_check("zero_n", flags, 0, false), "zero_n", "holds 4 bodies");
    refused(empty.table_check("no_bodies", flags, 4, false), "no_bodies", "holds 0 bodies");
    refused(ready.table_check("byte_two", two, 4, false), "byte_two", "reserved");
    refused(ready.table_check("byte_high", high, 4, false), "byte_high", "reserved");
    // ... and the getter
    accepted(ready.table_check("ok_get", out, 4, true), "a getter of the body count");
    accepted(empty.table_check("ok_get_empty", nullptr, 0, true), "a getter on a world without bodies");
    accepted(ready.table_check("ok_get_any_bytes", two, 4, true), "a getter does not read its array");
    refused(ready.table_check("get_null", nullptr, 4, true), "get_null", "NULL is_sensor");
    refused(ready.table_check("get_null_zero", nullptr, 0, true), "get_null_zero", "holds 4 bodies");
    refused(ready.table_check("get_short", out, 3, true), "get_short", "holds 4 bodies");

    // ---- the occupancy
    uint32_t sensors[2] = {}, offsets[3] = {}, n_out = 0;
    xpbd_sensor_hit hits[8] = {};
    accepted(ready.overlaps_check("ok_host", sensors, offsets, hits, 8, &n_out, true), "the host variant");
    accepted(ready.overlaps_check("ok_host_count_only", sensors, offsets, nullptr, 0, &n_out, true), "no hits with cap 0");
    accepted(ready.overlaps_check("ok_device", sensors, offsets, hits, 8, nullptr, false), "the device variant has no n_out");
    refused(ready.overlaps_check("null_sensors", nullptr, offsets, hits, 8, &n_out, true), "null_sensors", "NULL sensors or offsets");
    refused(ready.overlaps_check("null_offsets", sensors, nullptr, hits, 8, &n_out, true), "null_offsets", "NULL sensors or offsets");
    refused(ready.overlaps_check("null_hits", sensors, offsets, nullptr, 8, &n_out, true), "null_hits", "NULL hits");
    refused(ready.overlaps_check("null_n_out", sensors, offsets, hits, 8, nullptr, true), "null_n_out", "NULL n_out");
    refused(ready.overlaps_check("dev_null_offsets", sensors, nullptr, hits, 8, nullptr, false), "dev_null_offsets", "NULL sensors or offsets");
    refused(ready.overlaps_check("dev_null_hits", sensors, offsets, nullptr, 1, nullptr, false), "dev_null_hits", "NULL hits");
    refused(none.overlaps_check("no_sensor", sensors, offsets, hits, 8, &n_out, true), "no_sensor", "no sensor is set");
    refused(off.overlaps_check("reports_off", sensors, offsets, hits, 8, &n_out, true), "reports_off", "reports are off");
    refused(no_frame.overlaps_check("no_frame", sensors, offsets, hits, 8, &n_out, true), "no_frame", "no report");
    refused(no_frame.overlaps_check("dev_no_frame", sensors, offsets, hits, 8, nullptr, false), "dev_no_frame", "no report");

    // a table as long as a large world: every byte is read, none behind it
    std::vector<uint8_t> big(100000, 1);
    const SensorTarget large{100000, 0, true, true};
    accepted(large.table_check("ok_large", big.data(), 100000, false, &count), "a large table");
    expect(count == 100000, "ok_large: every byte is 1");
    big.back() = 4;
    refused(large.table_check("large_last_byte", big.data(), 100000, false), "large_last_byte", "is_sensor[99999]");

    if (failures)
        return 1;
    std::printf("%d checks ok\n", calls);
    return 0;
}
