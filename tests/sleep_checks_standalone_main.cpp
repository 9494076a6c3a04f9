// sleep_checks_standalone_main.cpp -- SleepTarget (csrc/xpbd_checks.cpp, declared in csrc/xpbd_checks.hpp), the argument checks
// of xpbd_world_set_sleeping, xpbd_world_sleep_state(_device) and xpbd_world_wake_bodies(_device), built with plain g++ (no
// hipcc, no ROCm include path; see test_sleep_model.py): every way they refuse a call, each with XPBD_E_INVALID and a message
// that names the `who` it was given, and the calls they accept.  Exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

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

xpbd_sleep_config config(double linear, double angular, uint32_t frames, uint32_t flags)
{
    xpbd_sleep_config c;
    c.linear_speed = linear;
    c.angular_speed = angular;
    c.frames_to_sleep = frames;
    c.flags = flags;
    return c;
}

} // namespace

int main()
{
    using namespace xpbd;
    static_assert(sizeof(xpbd_sleep_config) == 24, "xpbd_sleep_config is 24 bytes");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const SleepTarget ready{XPBD_MODE_CONTACTS, 4, true, false}, on{XPBD_MODE_CONTACTS, 4, true, true}, fused{XPBD_MODE_FUSED, 4, true, false},
        per_substep{XPBD_MODE_PER_SUBSTEP, 4, true, false}, no_report{XPBD_MODE_CONTACTS, 4, false, false}, empty{XPBD_MODE_CONTACTS, 0, true, true};

    accepted(ready.check("ok", config(0.1, 0.5, 30, 0)), "a usual configuration");
    accepted(ready.check("ok_zero", config(0.0, 0.0, 1, 0)), "zero thresholds, one frame");
    accepted(on.check("ok_again", config(1e300, 1e300, 0xFFFFFFFFu, 0)), "a new configuration while on");
    accepted(empty.check("ok_no_bodies", config(0.1, 0.5, 30, 0)), "a world without bodies yet");
    refused(ready.check("neg_linear", config(-0.1, 0.5, 30, 0)), "neg_linear", "linear_speed");
    refused(ready.check("inf_linear", config(inf, 0.5, 30, 0)), "inf_linear", "linear_speed");
    refused(ready.check("nan_linear", config(nan, 0.5, 30, 0)), "nan_linear", "linear_speed");
    refused(ready.check("neg_angular", config(0.1, -0.5, 30, 0)), "neg_angular", "angular_speed");
    refused(ready.check("inf_angular", config(0.1, inf, 30, 0)), "inf_angular", "angular_speed");
    refused(ready.check("nan_angular", config(0.1, nan, 30, 0)), "nan_angular", "angular_speed");
    refused(ready.check("no_frames", config(0.1, 0.5, 0, 0)), "no_frames", "frames_to_sleep");
    refused(ready.check("flag_1", config(0.1, 0.5, 30, 1u)), "flag_1", "unknown flags");
    refused(fused.check("mode_fused", config(0.1, 0.5, 30, 0)), "mode_fused", "XPBD_MODE_CONTACTS");
    refused(per_substep.check("mode_per_substep", config(0.1, 0.5, 30, 0)), "mode_per_substep", "XPBD_MODE_CONTACTS");
    refused(no_report.check("report_off", config(0.1, 0.5, 30, 0)), "report_off", "contact report");

    const uint32_t inside[3] = {0, 3, 3}, outside[3] = {0, 4, 1};
    accepted(on.state_check("state_ok"), "the state calls with sleeping on");
    refused(ready.state_check("state_off"), "state_off", "sleeping is off");
    accepted(on.wake_check("wake_ok", inside, 3), "a list, an index twice");
    accepted(on.wake_check("wake_all", nullptr, 0), "NULL with n == 0: everybody");
    accepted(on.wake_check("wake_none", inside, 0), "an empty list");
    refused(ready.wake_check("wake_off", inside, 3), "wake_off", "sleeping is off");
    refused(on.wake_check("wake_null", nullptr, 3), "wake_null", "NULL indices");
    refused(on.wake_check("wake_range", outside, 3), "wake_range", "indices[1] = 4");
    refused(empty.wake_check("wake_empty_world", inside, 1), "wake_empty_world", "holds 0 bodies");

    if (failures)
        return 1;
    std::printf("%d calls ok\n", calls);
    return 0;
}
