// joint_state_standalone_main.cpp -- the host-only parts of the joint states and drive targets, built with plain g++ (no hipcc, no
// ROCm include path; see test_joint_state_abi.py):
//   1. JointStateTarget::check and DriveTargets::check (csrc/xpbd_checks.cpp): every way the four calls refuse their arguments before
//      any device work, each with XPBD_E_INVALID and a message naming the `who` it was given, and the calls they accept;
//   2. the drive -> item map of build_extra_tables (csrc/xpbd_population_remap.cpp) against a naive restatement, on a crafted
//      case (drives in scrambled joint order, SLIDE limits interleaved, joints with two drives) and on 1 000 random ones.
// Exits 0.
#include <algorithm>
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

void check_calls()
{
    using namespace xpbd;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    xpbd_joint_state out[4] = {};
    const uint32_t some[3] = {2, 0, 2}, past[2] = {1, 4};
    // xpbd_world_joint_states against a world of 4 joints
    accepted(JointStateTarget{4}.check("ok_all", nullptr, 4, out, true), "all joints");
    accepted(JointStateTarget{4}.check("ok_some", some, 3, out, true), "a list, an index twice");
    accepted(JointStateTarget{0}.check("ok_none", nullptr, 0, nullptr, true), "a world without joints, n == 0");
    accepted(JointStateTarget{4}.check("ok_empty_list", some, 0, nullptr, true), "an empty list");
    accepted(JointStateTarget{4}.check("ok_device_range", past, 2, out, false), "the device variant does not read its list");
    refused(JointStateTarget{4}.check("null_out", nullptr, 4, nullptr, true), "null_out", "NULL out");
    refused(JointStateTarget{4}.check("null_out_device", some, 3, nullptr, false), "null_out_device", "NULL out");
    refused(JointStateTarget{4}.check("all_but_n", nullptr, 3, out, true), "all_but_n", "joints == NULL");
    refused(JointStateTarget{4}.check("all_but_n_device", nullptr, 5, out, false), "all_but_n_device", "joints == NULL");
    refused(JointStateTarget{0}.check("all_of_none", nullptr, 1, out, true), "all_of_none", "joints == NULL");
    refused(JointStateTarget{4}.check("range", past, 2, out, true), "range", "joints[1] = 4");

    // xpbd_world_set_drive_targets against three resident drives: ANGULAR_VELOCITY, ANGLE, POSITION
    xpbd_joint_drive resident[3] = {};
    resident[0].kind = XPBD_DRIVE_ANGULAR_VELOCITY;
    resident[1].kind = XPBD_DRIVE_ANGLE;
    resident[2].kind = XPBD_DRIVE_POSITION;
    const double good[3] = {40.0, -M_PI, 7.0}, bad_nan[3] = {1.0, 0.5, nan}, bad_inf[3] = {-inf, 0.5, 0.0}, bad_angle[3] = {4.0, 4.0, 4.0}, small[2] = {0.5, -0.5};
    const uint32_t two[2] = {0, 2}, twice[2] = {1, 1}, down[2] = {2, 0}, far[2] = {1, 3}, angle_only[1] = {1};
    accepted(DriveTargets{resident, 3}.check("ok_all", nullptr, good, 3, true), "all drives");
    accepted(DriveTargets{resident, 3}.check("ok_two", two, bad_angle, 2, true), "4.0 is fine for the kinds that are no ANGLE");
    accepted(DriveTargets{resident, 0}.check("ok_none", nullptr, nullptr, 0, true), "a world without drives, n == 0");
    accepted(DriveTargets{nullptr, 3}.check("ok_device", down, bad_nan, 2, false), "the device variant reads neither array");
    refused(DriveTargets{resident, 3}.check("null_targets", two, nullptr, 2, true), "null_targets", "NULL targets");
    refused(DriveTargets{nullptr, 3}.check("null_targets_device", two, nullptr, 2, false), "null_targets_device", "NULL targets");
    refused(DriveTargets{resident, 3}.check("all_but_n", nullptr, good, 2, true), "all_but_n", "drives == NULL");
    refused(DriveTargets{nullptr, 3}.check("all_but_n_device", nullptr, good, 4, false), "all_but_n_device", "drives == NULL");
    refused(DriveTargets{resident, 3}.check("range", far, small, 2, true), "range", "drives[1] = 3");
    refused(DriveTargets{resident, 3}.check("twice", twice, small, 2, true), "twice", "does not ascend");
    refused(DriveTargets{resident, 3}.check("down", down, small, 2, true), "down", "does not ascend");
    refused(DriveTargets{resident, 3}.check("nan", nullptr, bad_nan, 3, true), "nan", "targets[2]");
    refused(DriveTargets{resident, 3}.check("inf", nullptr, bad_inf, 3, true), "inf", "targets[0]");
    refused(DriveTargets{resident, 3}.check("angle", angle_only, bad_angle, 1, true), "angle", "angle drive 1");
}

// What the map must be, restated: the items are grouped by joint in ascending order of the joints that have any; inside a
// joint its SLIDE limit comes first, then its drives in the caller's order.
std::vector<uint32_t> naive_drive_items(const std::vector<xpbd_joint> &joints, const std::vector<xpbd_joint_limit> &slide,
                                        const std::vector<xpbd_joint_drive> &drives)
{
    std::vector<uint32_t> out(drives.size());
    uint32_t item = 0;
    for (uint32_t j = 0; j < joints.size(); ++j) {
        for (const xpbd_joint_limit &l : slide)
            item += l.joint == j;
        for (size_t d = 0; d < drives.size(); ++d)
            if (drives[d].joint == j)
                out[d] = item++;
    }
    return out;
}

bool map_holds(const std::vector<xpbd_joint> &joints, const std::vector<xpbd_joint_limit> &slide, const std::vector<xpbd_joint_drive> &drives,
               uint32_t n_bodies, const char *what)
{
    const xpbd::ExtraTables t = xpbd::build_extra_tables(joints, slide, drives, n_bodies);
    bool ok = t.drive_item == naive_drive_items(joints, slide, drives);
    for (size_t d = 0; ok && d < drives.size(); ++d) { // ... and the item is the drive, bit for bit
        ok = t.drive_item[d] < t.items.size() && std::memcmp(&t.items[t.drive_item[d]], &drives[d], sizeof drives[d]) == 0;
        const uint32_t *slot = nullptr; // the joint's range of items holds it
        for (size_t k = 0; k < t.list.size(); ++k)
            if (t.list[k] == drives[d].joint)
                slot = &t.off[k];
        ok = ok && slot && slot[0] <= t.drive_item[d] && t.drive_item[d] < slot[1];
    }
    if (!ok) {
        ++failures;
        std::printf("%s: the drive -> item map is wrong\n", what);
    }
    return ok;
}

xpbd_joint joint_of(uint32_t a, uint32_t b, uint32_t kind)
{
    xpbd_joint j{};
    j.body_a = a, j.body_b = b, j.kind = kind;
    j.axis_a[2] = j.axis_b[2] = 1.0;
    return j;
}

xpbd_joint_drive drive_of(uint32_t joint, uint32_t kind, double target)
{
    xpbd_joint_drive d{};
    d.joint = joint, d.kind = kind, d.target = target, d.max_force = 1.0;
    d.ref_a[0] = d.ref_b[0] = 1.0;
    return d;
}

xpbd_joint_limit slide_of(uint32_t joint)
{
    xpbd_joint_limit l{};
    l.joint = joint, l.kind = XPBD_LIMIT_SLIDE, l.lower = -1.0, l.upper = 1.0;
    return l;
}

void crafted_case()
{
    // joints 0..5 on a chain of 7 bodies: hinge, slider, ball, slider, hinge, slider (the last without limit or drive: listed for
    // its perpendicular term alone)
    std::vector<xpbd_joint> joints;
    const uint32_t kinds[6] = {XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER, XPBD_JOINT_DISTANCE, XPBD_JOINT_SLIDER, XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER};
    for (uint32_t k = 0; k < 6; ++k)
        joints.push_back(joint_of(k, k + 1, kinds[k]));
    const std::vector<xpbd_joint_limit> slide = {slide_of(3), slide_of(1)};
    // scrambled joint order; joints 1 and 3 carry two drives each, given in opposite orders
    const std::vector<xpbd_joint_drive> drives = {drive_of(4, XPBD_DRIVE_ANGLE, 0.1),    drive_of(3, XPBD_DRIVE_VELOCITY, 0.2),
                                                  drive_of(1, XPBD_DRIVE_ANGLE, 0.3),    drive_of(0, XPBD_DRIVE_ANGULAR_VELOCITY, 0.4),
                                                  drive_of(3, XPBD_DRIVE_ANGLE, 0.5),    drive_of(1, XPBD_DRIVE_POSITION, 0.6)};
    // items: [0] drive 3 | [1] slide 1, [2] drive 2, [3] drive 5 | [4] slide 3, [5] drive 1, [6] drive 4 | [7] drive 0 | joint 5: none
    const std::vector<uint32_t> want = {7, 5, 2, 0, 6, 3};
    const xpbd::ExtraTables t = xpbd::build_extra_tables(joints, slide, drives, 7);
    ++calls;
    if (t.drive_item != want || t.list != std::vector<uint32_t>{0, 1, 3, 4, 5} || t.off != std::vector<uint32_t>{0, 1, 4, 7, 8, 8}) {
        ++failures;
        std::printf("crafted case: the tables are not the ones written down\n");
    }
    map_holds(joints, slide, drives, 7, "crafted case");
    // no drives at all: an empty map, with or without other extras
    ++calls;
    if (!xpbd::build_extra_tables(joints, slide, {}, 7).drive_item.empty() || !xpbd::build_extra_tables({}, {}, {}, 0).drive_item.empty()) {
        ++failures;
        std::printf("no drives: the map is not empty\n");
    }
}

void random_cases()
{
    std::mt19937 rng(20240611u);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    for (int c = 0; c < 1000; ++c) {
        const uint32_t n_bodies = 2 + below(30), n_joints = below(40);
        std::vector<xpbd_joint> joints;
        for (uint32_t k = 0; k < n_joints; ++k) {
            const uint32_t a = below(n_bodies);
            joints.push_back(joint_of(a, (a + 1 + below(n_bodies - 1)) % n_bodies, below(3)));
        }
        std::vector<xpbd_joint_limit> slide;
        std::vector<xpbd_joint_drive> drives;
        for (uint32_t k = 0; k < n_joints; ++k) { // what the setters accept: at most one SLIDE limit, one angular, one linear drive
            const bool slider = joints[k].kind == XPBD_JOINT_SLIDER;
            if (slider && below(2))
                slide.push_back(slide_of(k));
            if (joints[k].kind != XPBD_JOINT_DISTANCE && below(2))
                drives.push_back(drive_of(k, below(2) ? XPBD_DRIVE_ANGLE : XPBD_DRIVE_ANGULAR_VELOCITY, 0.001 * c + k));
            if (slider && below(2))
                drives.push_back(drive_of(k, below(2) ? XPBD_DRIVE_POSITION : XPBD_DRIVE_VELOCITY, -0.001 * c - k));
        }
        std::shuffle(slide.begin(), slide.end(), rng);
        std::shuffle(drives.begin(), drives.end(), rng);
        if (!map_holds(joints, slide, drives, n_bodies, "random case"))
            return;
    }
    ++calls;
}

} // namespace

int main()
{
    check_calls();
    crafted_case();
    random_cases();
    if (failures)
        return 1;
    std::printf("%d checks ok, 1000 random cases ok\n", calls);
    return 0;
}
