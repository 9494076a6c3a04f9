// checks_standalone_main.cpp -- csrc/xpbd_checks.cpp and csrc/xpbd_error.cpp built with plain g++ (no hipcc, no ROCm include
// path; see test_checks_standalone.py): every check_* function accepts one call and refuses one, with XPBD_E_INVALID and a
// message that names the `who` it was given.  Exits 0.
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

void refused(int rc, const char *who)
{
    ++calls;
    if (rc != XPBD_E_INVALID || !std::strstr(xpbd_last_error(), who)) {
        ++failures;
        std::printf("%s: refused call returned %d with message '%s'\n", who, rc, xpbd_last_error());
    }
}

xpbd_joint hinge(uint32_t a, uint32_t b)
{
    xpbd_joint j{};
    j.body_a = a;
    j.body_b = b;
    j.kind = XPBD_JOINT_HINGE;
    j.axis_a[2] = j.axis_b[2] = 1.0;
    return j;
}

} // namespace

int main()
{
    using namespace xpbd;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const QueryTarget world{true, 4, 2, "the_setter", true, true}, bare{false, 4, 2, "the_setter", false, false};

    accepted(check_query_flags("flags_ok", world, XPBD_QUERY_TERRAIN | 1u, 1u), "check_query_flags");
    refused(check_query_flags("flags_bad", bare, XPBD_QUERY_TERRAIN, 1u), "flags_bad");

    xpbd_ray ray{};
    xpbd_ray_hit ray_hit{};
    accepted(check_raycast("raycast_ok", world, &ray, 1, XPBD_RAYCAST_BRUTE_FORCE, &ray_hit, true), "check_raycast");
    ray.reserved = 7;
    refused(check_raycast("raycast_bad", world, &ray, 1, 0, &ray_hit, true), "raycast_bad");

    xpbd_overlap_query query{};
    xpbd_overlap_hit overlap_hit{};
    uint32_t offsets[2] = {0, 0}, n_out = 0;
    query.shape = 1;
    accepted(check_overlap("overlap_ok", world, &query, 1, XPBD_OVERLAP_MASKED, offsets, &overlap_hit, 1, &n_out, true), "check_overlap");
    query.shape = 2; // of 2 shapes
    refused(check_overlap("overlap_bad", world, &query, 1, 0, offsets, &overlap_hit, 1, &n_out, true), "overlap_bad");

    xpbd_sweep sweep{};
    xpbd_sweep_hit sweep_hit{};
    accepted(check_sweep("sweep_ok", world, &sweep, 1, XPBD_SWEEP_BRUTE_FORCE, &sweep_hit, true), "check_sweep");
    refused(check_sweep("sweep_bad", bare, &sweep, 1, 0, &sweep_hit, true), "sweep_bad"); // no polytopes

    xpbd_distance_query distance{};
    xpbd_distance_hit distance_hit{};
    distance.shape = XPBD_DISTANCE_POINT;
    accepted(check_distance("distance_ok", world, &distance, 1, XPBD_DISTANCE_MASKED, &distance_hit, true), "check_distance");
    refused(check_distance("distance_bad", world, &distance, 1, XPBD_QUERY_TERRAIN, &distance_hit, true), "distance_bad"); // the terrain is no body

    const QueryTarget flat{true, 4, 2, "the_setter", true, false}; // no terrain
    accepted(check_terrain_distance("terrain_distance_ok", world, &distance, 1, XPBD_DISTANCE_BRUTE_FORCE, &distance_hit, true), "check_terrain_distance");
    refused(check_terrain_distance("terrain_distance_bad", flat, &distance, 1, 0, &distance_hit, true), "terrain_distance_bad");

    xpbd_joint joints[2] = {hinge(0, 1), hinge(1, 2)};
    accepted(check_joints("joints_ok", joints, 2, 3), "check_joints");
    refused(check_joints("joints_bad", joints, 2, 2), "joints_bad"); // body 2 of 2

    xpbd_joint_limit limit{};
    limit.joint = 1;
    limit.kind = XPBD_LIMIT_HINGE;
    limit.ref_a[0] = limit.ref_b[0] = 1.0;
    limit.lower = -0.5;
    limit.upper = 0.5;
    accepted(check_joint_limits("limits_ok", joints, 2, &limit, 1), "check_joint_limits");
    limit.upper = 4.0; // > pi
    refused(check_joint_limits("limits_bad", joints, 2, &limit, 1), "limits_bad");

    xpbd_joint_drive drive{};
    drive.joint = 0;
    drive.kind = XPBD_DRIVE_ANGULAR_VELOCITY;
    drive.ref_a[1] = drive.ref_b[1] = 1.0;
    drive.target = 2.0;
    drive.max_force = std::numeric_limits<double>::infinity();
    accepted(check_joint_drives("drives_ok", joints, 2, &drive, 1), "check_joint_drives");
    drive.kind = XPBD_DRIVE_POSITION; // needs a slider
    refused(check_joint_drives("drives_bad", joints, 2, &drive, 1), "drives_bad");

    const double values[4] = {0.0, 1.0, 2.0, nan};
    accepted(check_per_body("per_body_ok", "values", values, 4, 4), "check_per_body");
    refused(check_per_body("per_body_bad", "values", values, 3, 4), "per_body_bad");

    xpbd_material materials[2] = {{0.5, 0.0}, {std::numeric_limits<double>::infinity(), 0.0}};
    accepted(check_materials("materials_ok", materials, 2), "check_materials");
    materials[1].friction = nan;
    refused(check_materials("materials_bad", materials, 2), "materials_bad");

    const uint32_t indices[3] = {2, 0, 2};
    accepted(check_edit_indices("indices_ok", indices, 3, 3, false), "check_edit_indices");
    refused(check_edit_indices("indices_bad", indices, 3, 3, true), "indices_bad"); // 2 listed twice

    accepted(check_edit_finite("finite_ok", "values", values, 3), "check_edit_finite");
    refused(check_edit_finite("finite_bad", "values", values, 4), "finite_bad");

    xpbd_impulse impulse{};
    impulse.body = 3;
    impulse.flags = XPBD_IMPULSE_AT_CENTRE;
    impulse.point[0] = nan; // ignored at the centre
    accepted(check_impulses("impulses_ok", &impulse, 1, 4), "check_impulses");
    impulse.flags = XPBD_IMPULSE_AT_POINT;
    refused(check_impulses("impulses_bad", &impulse, 1, 4), "impulses_bad");

    if (failures)
        return 1;
    std::printf("%d calls ok\n", calls);
    return 0;
}
