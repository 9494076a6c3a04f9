// damping_checks_standalone_main.cpp -- DampingTarget (csrc/xpbd_checks.cpp, declared in csrc/xpbd_checks.hpp), the argument checks of xpbd_world_set_damping, _get_damping and _set_joint_damping, and
// remap_joint_set with the fourth vector of xpbd::JointSet plus build_joint_damping_table (csrc/xpbd_population_remap.cpp), built
// with plain g++ (no hipcc, no ROCm include path; see test_damping_checks_standalone.py): every way the checks refuse a call,
// each with XPBD_E_INVALID and a message that names the `who` it was given, the calls they accept, and the re-index against a
// restatement on random joint sets.  Exits 0.
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

void expect(bool ok, const char *what)
{
    ++calls;
    if (!ok) {
        ++failures;
        std::printf("%s: wrong\n", what);
    }
}

xpbd_joint_damping damper(uint32_t joint, double linear, double angular)
{
    xpbd_joint_damping d;
    d.joint = joint;
    d.reserved = 0;
    d.linear = linear;
    d.angular = angular;
    return d;
}

} // namespace

int main()
{
    using namespace xpbd;
    static_assert(sizeof(xpbd_body_damping) == 32 && sizeof(xpbd_joint_damping) == 24, "the records of include/xpbd.h");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const xpbd_body_damping dflt{0.0, 0.0, inf, inf};
    const DampingTarget world{4, 5}, empty{0, 0};

    // ---- xpbd_world_set_damping / _get_damping: the rows ----
    std::vector<xpbd_body_damping> rows(4, dflt);
    bool any = true;
    accepted(world.rows("ok_default", nullptr, 0), "NULL with n == 0: all defaults");
    accepted(world.rows("ok_all_default", rows.data(), 4, &any), "default rows");
    expect(!any, "default rows set nothing");
    accepted(empty.rows("ok_null", nullptr, 0, &any), "no rows, no bodies");
    expect(!any, "no rows set nothing");
    for (int field = 0; field < 4; ++field) { // each field alone turns the pass on
        std::vector<xpbd_body_damping> r = rows;
        (field == 0 ? r[2].linear : field == 1 ? r[2].angular : field == 2 ? r[2].max_linear_speed : r[2].max_angular_speed) = 2.5;
        any = false;
        accepted(world.rows("ok_one_field", r.data(), 4, &any), "one field set");
        expect(any, "one field differs from the default");
    }
    {
        std::vector<xpbd_body_damping> r = rows;
        r[0].linear = r[0].angular = -0.0;
        r[3].max_linear_speed = 5e-324;
        accepted(world.rows("ok_edges", r.data(), 4), "-0.0 coefficients, the smallest positive cap");
    }
    refused(world.rows("null_rows", nullptr, 4), "null_rows", "NULL rows");
    refused(world.rows("count", rows.data(), 3), "count", "holds 4 bodies");
    refused(world.rows("count_more", rows.data(), 5), "count_more", "holds 4 bodies");
    for (double bad : {-1.0, -1e-300, nan, inf, -inf}) {
        std::vector<xpbd_body_damping> r = rows;
        r[1].linear = bad;
        refused(world.rows("linear", r.data(), 4), "linear", "rows[1].linear");
        r = rows;
        r[3].angular = bad;
        refused(world.rows("angular", r.data(), 4), "angular", "rows[3].angular");
    }
    for (double bad : {0.0, -0.0, -3.0, nan, -inf}) {
        std::vector<xpbd_body_damping> r = rows;
        r[0].max_linear_speed = bad;
        refused(world.rows("linear_cap", r.data(), 4), "linear_cap", "rows[0].max_linear_speed");
        r = rows;
        r[2].max_angular_speed = bad;
        refused(world.rows("angular_cap", r.data(), 4), "angular_cap", "rows[2].max_angular_speed");
    }

    // ---- xpbd_world_set_joint_damping: the list against a world of five joints ----
    std::vector<xpbd_joint_damping> list = {damper(3, 1.0, 0.0), damper(0, 0.0, 2.0), damper(4, 0.0, 0.0)};
    accepted(world.dampers("ok_list", list.data(), 3), "three joints in any order");
    accepted(world.dampers("ok_clear", nullptr, 0), "n == 0 clears");
    accepted(empty.dampers("ok_clear_no_joints", nullptr, 0), "clearing a world without joints");
    refused(world.dampers("null_list", nullptr, 2), "null_list", "NULL list");
    refused(empty.dampers("no_joints", list.data(), 1), "no_joints", "names joint 3 of 0");
    {
        std::vector<xpbd_joint_damping> l = list;
        l[1].joint = 5;
        refused(world.dampers("range", l.data(), 3), "range", "list[1] names joint 5 of 5");
        l = list;
        l[2].joint = 3;
        refused(world.dampers("twice", l.data(), 3), "twice", "second entry for joint 3");
        l = list;
        l[0].reserved = 1;
        refused(world.dampers("reserved", l.data(), 3), "reserved", "reserved must be 0");
        for (double bad : {-1.0, nan, inf, -inf}) {
            l = list;
            l[0].linear = bad;
            refused(world.dampers("mu_linear", l.data(), 3), "mu_linear", "list[0].linear");
            l = list;
            l[2].angular = bad;
            refused(world.dampers("mu_angular", l.data(), 3), "mu_angular", "list[2].angular");
        }
    }

    // ---- the dense table ----
    {
        const std::vector<double> t = build_joint_damping_table(list, 5);
        const double want[10] = {0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
        expect(t.size() == 10 && std::memcmp(t.data(), want, sizeof want) == 0, "the table of three entries");
        expect(build_joint_damping_table({damper(1, 0.0, 0.0), damper(2, -0.0, 0.0)}, 5).empty(), "only zero coefficients: off");
        expect(build_joint_damping_table({}, 5).empty(), "an empty list: off");
    }
    const int checks = calls;

    // ---- the population re-index, with the fourth vector ----
    std::mt19937 rng(5400);
    int cases = 0;
    for (; cases < 1000; ++cases) {
        const uint32_t n_bodies = 2 + rng() % 30, n_joints = rng() % 25;
        std::vector<uint32_t> map(n_bodies);
        uint32_t next = 0;
        for (uint32_t i = 0; i < n_bodies; ++i)
            map[i] = rng() % 4 == 0 ? kRemoved : next++;
        JointSet in;
        for (uint32_t k = 0; k < n_joints; ++k) {
            xpbd_joint j{};
            j.body_a = rng() % n_bodies;
            do
                j.body_b = rng() % n_bodies;
            while (j.body_b == j.body_a);
            j.distance = (double)k;
            in.joints.push_back(j);
        }
        std::vector<uint32_t> order(n_joints);
        for (uint32_t k = 0; k < n_joints; ++k)
            order[k] = k;
        for (uint32_t k = n_joints; k > 1; --k)
            std::swap(order[k - 1], order[rng() % k]);
        for (uint32_t k : order)
            if (rng() % 2)
                in.damping.push_back(damper(k, 0.5 + k, 100.0 + k));
        if (n_joints) { // a limit and a drive as before: the other vectors are not disturbed
            xpbd_joint_limit l{};
            l.joint = rng() % n_joints;
            in.limits.push_back(l);
            xpbd_joint_drive d{};
            d.joint = rng() % n_joints;
            in.drives.push_back(d);
        }
        std::vector<uint32_t> joint_map;
        const JointSet out = remap_joint_set(in, map.data(), n_bodies, joint_map);
        // restatement: a joint survives iff both ends do; survivors are numbered in order
        std::vector<uint32_t> want_map(n_joints, kRemoved);
        uint32_t kept = 0;
        for (uint32_t k = 0; k < n_joints; ++k)
            if (map[in.joints[k].body_a] != kRemoved && map[in.joints[k].body_b] != kRemoved)
                want_map[k] = kept++;
        bool ok = joint_map == want_map && out.joints.size() == kept;
        size_t at = 0;
        for (const xpbd_joint_damping &d : in.damping) {
            if (want_map[d.joint] == kRemoved)
                continue;
            ok = ok && at < out.damping.size() && out.damping[at].joint == want_map[d.joint] && out.damping[at].reserved == 0 &&
                 out.damping[at].linear == d.linear && out.damping[at].angular == d.angular &&
                 out.joints[out.damping[at].joint].distance == (double)d.joint; // ... and names the joint it named before
            ++at;
        }
        ok = ok && at == out.damping.size();
        ok = ok && out.limits.size() == (n_joints && want_map[in.limits[0].joint] != kRemoved ? 1u : 0u);
        ok = ok && out.drives.size() == (n_joints && want_map[in.drives[0].joint] != kRemoved ? 1u : 0u);
        // what comes out is a list xpbd_world_set_joint_damping would accept for the new joints
        ok = ok && (DampingTarget{next, kept}.dampers("remapped", out.damping.data(), (uint32_t)out.damping.size())) == XPBD_OK;
        if (!ok) {
            ++failures;
            std::printf("remap_joint_set: case %d is wrong\n", cases);
            break;
        }
    }
    if (failures)
        return 1;
    std::printf("%d checks ok, %d random re-index cases ok\n", checks, cases);
    return 0;
}
