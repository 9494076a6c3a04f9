// kinematic_checks_standalone_main.cpp -- KinematicTarget and KinematicTargets (csrc/xpbd_checks.cpp, declared in
// csrc/xpbd_checks.hpp), the argument checks of xpbd_world_set_kinematics and xpbd_world_set_kinematic_targets(_device), and
// remap_kinematics (csrc/xpbd_population_remap.cpp), the re-index of the table by a population change, built with plain g++ (no
// hipcc, no ROCm include path; see test_kinematic_checks_standalone.py): every way the checks refuse a call, each with
// XPBD_E_INVALID and a message that names the `who` it was given, the calls they accept, and the re-index against a restatement
// on random tables.  Exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_checks.hpp"
#include "../constraint_solver_amd/csrc/xpbd_population_remap.hpp"

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

xpbd_kinematic entry(uint32_t body, uint32_t mode, double x = 0.0)
{
    xpbd_kinematic e;
    e.body = body;
    e.mode = mode;
    e.linear[0] = x;
    e.linear[1] = 2.0;
    e.linear[2] = 3.0;
    e.angular[0] = mode == XPBD_KINEMATIC_POSE ? 1.0 : 0.0;
    e.angular[1] = e.angular[2] = e.angular[3] = 0.0;
    return e;
}

} // namespace

int main()
{
    using namespace xpbd;
    static_assert(sizeof(xpbd_kinematic) == 64, "xpbd_kinematic is 64 bytes");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const KinematicTarget world{8}, empty{0};

    // ---- xpbd_world_set_kinematics ----
    std::vector<xpbd_kinematic> good = {entry(1, XPBD_KINEMATIC_POSE), entry(2, XPBD_KINEMATIC_VELOCITY), entry(7, XPBD_KINEMATIC_POSE)};
    accepted(world.check("ok", good.data(), 3), "an ascending table of both modes");
    accepted(world.check("ok_clear", nullptr, 0), "NULL with n == 0 clears");
    accepted(empty.check("ok_clear_empty", nullptr, 0), "clearing a world without bodies");
    {
        std::vector<xpbd_kinematic> t = good;
        t[1].linear[0] = t[1].linear[1] = t[1].linear[2] = t[1].angular[0] = t[1].angular[1] = t[1].angular[2] = 0.0;
        accepted(world.check("ok_zero_velocity", t.data(), 3), "an all-zero VELOCITY entry");
        t[0].angular[0] = 0.0;
        t[0].angular[3] = -2.5;
        accepted(world.check("ok_unnormalised", t.data(), 3), "a POSE rotation that is not unit");
    }
    refused(world.check("null_list", nullptr, 3), "null_list", "NULL list");
    refused(empty.check("no_bodies", good.data(), 1), "no_bodies", "holds no bodies");
    {
        std::vector<xpbd_kinematic> t = good;
        t[2].body = 8;
        refused(world.check("range", t.data(), 3), "range", "list[2].body = 8");
        t = good;
        t[1].body = 1;
        refused(world.check("repeat", t.data(), 3), "repeat", "does not ascend");
        t = good;
        t[2].body = 0;
        refused(world.check("descent", t.data(), 3), "descent", "does not ascend");
        t = good;
        t[1].mode = 2;
        refused(world.check("mode", t.data(), 3), "mode", "unknown mode 2");
        for (uint32_t c = 0; c < 7; ++c) {
            for (double bad : {nan, inf, -inf}) {
                t = good;
                (c < 3 ? t[c % 3].linear[c] : t[c % 3].angular[c - 3]) = bad;
                refused(world.check("finite", t.data(), 3), "finite", "must be finite");
            }
        }
        t = good;
        t[1].angular[3] = nan; // ignored by the step, checked all the same
        refused(world.check("finite_ignored", t.data(), 3), "finite_ignored", "angular[3]");
        t = good;
        t[0].angular[0] = 0.0;
        refused(world.check("zero_rotation", t.data(), 3), "zero_rotation", "all-zero target rotation");
        t = good;
        t[2].angular[0] = -0.0;
        refused(world.check("minus_zero_rotation", t.data(), 3), "minus_zero_rotation", "all-zero target rotation");
    }
    // the mass doubles of the named bodies: ten each
    {
        std::vector<double> mass(30, 0.0);
        accepted(world.fixed_check("ok_fixed", good.data(), 3, mass.data()), "three fixed bodies");
        mass[5] = -0.0;
        accepted(world.fixed_check("ok_minus_zero", good.data(), 3, mass.data()), "-0.0 is zero");
        mass[10] = 0.5;
        refused(world.fixed_check("has_mass", good.data(), 3, mass.data()), "has_mass", "list[1].body = 2 is not fixed (inverse_mass");
        mass[10] = 0.0;
        mass[29] = 1e-300;
        refused(world.fixed_check("has_inertia", good.data(), 3, mass.data()), "has_inertia", "list[2].body = 7 is not fixed (an inverse_inertia entry");
        mass[29] = nan;
        refused(world.fixed_check("nan_inertia", good.data(), 3, mass.data()), "nan_inertia", "is not fixed");
    }

    // ---- xpbd_world_set_kinematic_targets(_device) ----
    const KinematicTargets table{good.data(), 3}, device_side{nullptr, 3}, none{nullptr, 0};
    const uint32_t all[3] = {0, 1, 2}, two[2] = {0, 2}, repeat[2] = {1, 1}, down[2] = {2, 0}, outside[2] = {1, 3};
    double rows[21];
    for (int k = 0; k < 21; ++k)
        rows[k] = 0.25 * (k + 1);
    accepted(table.check("t_ok_all", nullptr, rows, 3, true), "NULL entries with n == the entry count");
    accepted(table.check("t_ok_list", all, rows, 3, true), "every entry listed");
    accepted(table.check("t_ok_two", two, rows, 2, true), "an ascending subset");
    accepted(table.check("t_ok_none", two, rows, 0, true), "an empty list");
    accepted(none.check("t_ok_no_table", nullptr, nullptr, 0, true), "no table, n == 0");
    accepted(device_side.check("t_ok_device", two, rows, 2, false), "the device variant reads neither list");
    accepted(device_side.check("t_ok_device_all", nullptr, rows, 3, false), "the device variant, all entries");
    refused(table.check("t_null_rows", two, nullptr, 2, true), "t_null_rows", "NULL rows");
    refused(device_side.check("t_null_rows_dev", two, nullptr, 2, false), "t_null_rows_dev", "NULL rows");
    refused(table.check("t_count", nullptr, rows, 2, true), "t_count", "holds 3 entries");
    refused(device_side.check("t_count_dev", nullptr, rows, 2, false), "t_count_dev", "holds 3 entries");
    refused(none.check("t_no_table", nullptr, rows, 1, true), "t_no_table", "holds 0 entries");
    refused(table.check("t_range", outside, rows, 2, true), "t_range", "entries[1] = 3");
    refused(table.check("t_repeat", repeat, rows, 2, true), "t_repeat", "does not ascend");
    refused(table.check("t_descent", down, rows, 2, true), "t_descent", "does not ascend");
    for (int c = 0; c < 7; ++c) {
        for (double bad : {nan, inf, -inf}) {
            double r[14];
            std::memcpy(r, rows, sizeof r);
            r[7 + c] = bad;
            refused(table.check("t_finite", two, r, 2, true), "t_finite", "must be finite");
        }
    }
    {
        double r[21];
        std::memcpy(r, rows, sizeof r);
        r[3] = r[4] = r[5] = r[6] = 0.0; // entry 0 is POSE
        refused(table.check("t_zero_rotation", nullptr, r, 3, true), "t_zero_rotation", "all-zero target rotation");
        std::memcpy(r, rows, sizeof r);
        r[7] = r[8] = r[9] = r[10] = r[11] = r[12] = r[13] = 0.0; // entry 1 is VELOCITY: all zero is standing still
        accepted(table.check("t_ok_zero_velocity", nullptr, r, 3, true), "a VELOCITY row of zeros");
    }
    refused(device_side.check("t_too_many", two, rows, (1u << 29) + 1u, false), "t_too_many", "2^29");
    refused(device_side.check("t_alignment", two, reinterpret_cast<const double *>(reinterpret_cast<const char *>(rows) + 4), 2, false), "t_alignment",
            "8-byte aligned");
    const int checks = calls;

    // ---- the population re-index ----
    std::mt19937 rng(4400);
    int cases = 0;
    for (; cases < 1000; ++cases) {
        const uint32_t n_bodies = 1 + rng() % 40;
        std::vector<uint32_t> map(n_bodies);
        uint32_t next = 0;
        for (uint32_t i = 0; i < n_bodies; ++i)
            map[i] = rng() % 3 == 0 ? kRemoved : next++;
        std::vector<xpbd_kinematic> in;
        for (uint32_t i = 0; i < n_bodies; ++i)
            if (rng() % 2)
                in.push_back(entry(i, rng() % 2, (double)i + 0.5));
        const std::vector<xpbd_kinematic> out = remap_kinematics(in, map.data(), n_bodies);
        size_t at = 0;
        bool ok = true;
        for (const xpbd_kinematic &e : in) {
            if (map[e.body] == kRemoved)
                continue;
            ok = ok && at < out.size() && out[at].body == map[e.body] && out[at].mode == e.mode &&
                 std::memcmp(out[at].linear, e.linear, 7 * sizeof(double)) == 0 && (at == 0 || out[at - 1].body < out[at].body);
            ++at;
        }
        ok = ok && at == out.size();
        if (ok && !out.empty()) // what comes out is a table xpbd_world_set_kinematics would accept for the new world
            ok = KinematicTarget{next}.check("remapped", out.data(), (uint32_t)out.size()) == XPBD_OK;
        if (!ok) {
            ++failures;
            std::printf("remap_kinematics: case %d is wrong\n", cases);
            break;
        }
    }
    {
        std::vector<xpbd_kinematic> stray = {entry(3, XPBD_KINEMATIC_POSE), entry(9, XPBD_KINEMATIC_POSE)}; // (never: an entry beyond the map is dropped, not read)
        const uint32_t map[4] = {0, kRemoved, 1, 2};
        const std::vector<xpbd_kinematic> out = remap_kinematics(stray, map, 4);
        if (out.size() != 1 || out[0].body != 2)
            ++failures;
    }

    if (failures)
        return 1;
    std::printf("%d checks ok, %d random re-index cases ok\n", checks, cases);
    return 0;
}
