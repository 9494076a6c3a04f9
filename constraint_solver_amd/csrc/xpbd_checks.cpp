// xpbd_checks.cpp -- the argument checks of the C ABI that need no device, shared by the single and the multi-GPU world.
// Host-only: no HIP header, builds with plain g++ (as xpbd_population_remap.cpp).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "xpbd_checks.hpp"
#include "xpbd_error.h"
#include "xpbd_mass_row.hpp"

namespace xpbd {

int check_joints(const char *who, const xpbd_joint *joints, uint32_t n_joints, uint32_t n_bodies)
{
    for (uint32_t k = 0; k < n_joints; ++k) {
        const xpbd_joint &j = joints[k];
        if (j.body_a >= n_bodies || j.body_b >= n_bodies || j.body_a == j.body_b)
            return set_error(XPBD_E_INVALID, "%s: joint %u links bodies %u and %u of %u", who, k, j.body_a, j.body_b, n_bodies);
        if (!(j.distance >= 0.0) || !(j.distance <= 1.0e300))
            return set_error(XPBD_E_INVALID, "%s: joint %u has distance %g", who, k, j.distance);
        if (j.kind != XPBD_JOINT_DISTANCE && j.kind != XPBD_JOINT_HINGE && j.kind != XPBD_JOINT_SLIDER)
            return set_error(XPBD_E_INVALID, "%s: joint %u has unknown kind %u", who, k, j.kind);
        if (j.kind == XPBD_JOINT_SLIDER && j.distance != 0.0)
            return set_error(XPBD_E_INVALID, "%s: slider %u needs distance 0 (got %g)", who, k, j.distance);
        if (j.reserved != 0)
            return set_error(XPBD_E_INVALID, "%s: joint %u: reserved must be 0", who, k);
        if (j.kind == XPBD_JOINT_HINGE || j.kind == XPBD_JOINT_SLIDER)
            for (const double *axis : {j.axis_a, j.axis_b}) {
                const double len2 = axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2];
                if (!(len2 > 0.999 && len2 < 1.001))
                    return set_error(XPBD_E_INVALID, "%s: %s %u needs unit axes (|axis|^2 = %g)", who, j.kind == XPBD_JOINT_HINGE ? "hinge" : "slider", k, len2);
            }
    }
    return XPBD_OK;
}

int check_per_body(const char *who, const char *what, const void *values, uint32_t n, uint32_t n_bodies, const char *count)
{
    if (!values && n)
        return set_error(XPBD_E_INVALID, "%s: NULL %s with %s = %u", who, what, count, n);
    if (values && n != n_bodies)
        return set_error(XPBD_E_INVALID, "%s: %s = %u but the world holds %u bodies", who, count, n, n_bodies);
    return XPBD_OK;
}

int check_materials(const char *who, const xpbd_material *materials, uint32_t n)
{
    for (uint32_t i = 0; materials && i < n; ++i) {
        if (!(materials[i].friction >= 0.0))
            return set_error(XPBD_E_INVALID, "%s: materials[%u].friction = %g (must be >= 0, +inf allowed)", who, i, materials[i].friction);
        if (!(materials[i].reserved == 0.0))
            return set_error(XPBD_E_INVALID, "%s: materials[%u].reserved = %g (must be 0)", who, i, materials[i].reserved);
    }
    return XPBD_OK;
}

int DampingTarget::rows(const char *who, const xpbd_body_damping *rows, uint32_t n, bool *any_set) const
{
    static_assert(sizeof(xpbd_body_damping) == 32, "xpbd_body_damping is {linear, angular, max_linear_speed, max_angular_speed}");
    if (int rc = check_per_body(who, "rows", rows, n, n_bodies))
        return rc;
    bool any = false;
    for (uint32_t i = 0; rows && i < n; ++i) {
        const xpbd_body_damping &r = rows[i];
        if (!(r.linear >= 0.0 && std::isfinite(r.linear)))
            return set_error(XPBD_E_INVALID, "%s: rows[%u].linear = %g (must be >= 0 and finite)", who, i, r.linear);
        if (!(r.angular >= 0.0 && std::isfinite(r.angular)))
            return set_error(XPBD_E_INVALID, "%s: rows[%u].angular = %g (must be >= 0 and finite)", who, i, r.angular);
        if (!(r.max_linear_speed > 0.0))
            return set_error(XPBD_E_INVALID, "%s: rows[%u].max_linear_speed = %g (must be > 0, +inf allowed)", who, i, r.max_linear_speed);
        if (!(r.max_angular_speed > 0.0))
            return set_error(XPBD_E_INVALID, "%s: rows[%u].max_angular_speed = %g (must be > 0, +inf allowed)", who, i, r.max_angular_speed);
        any = any || r.linear > 0.0 || r.angular > 0.0 || std::isfinite(r.max_linear_speed) || std::isfinite(r.max_angular_speed);
    }
    if (any_set)
        *any_set = any;
    return XPBD_OK;
}

int DampingTarget::dampers(const char *who, const xpbd_joint_damping *list, uint32_t n) const
{
    static_assert(sizeof(xpbd_joint_damping) == 24, "xpbd_joint_damping is {joint, reserved, linear, angular}");
    if (n && !list)
        return set_error(XPBD_E_INVALID, "%s: NULL list with n = %u", who, n);
    std::vector<uint8_t> seen(n_joints, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const xpbd_joint_damping &d = list[k];
        if (d.joint >= n_joints)
            return set_error(XPBD_E_INVALID, "%s: list[%u] names joint %u of %u", who, k, d.joint, n_joints);
        if (d.reserved != 0)
            return set_error(XPBD_E_INVALID, "%s: list[%u]: reserved must be 0", who, k);
        if (seen[d.joint])
            return set_error(XPBD_E_INVALID, "%s: list[%u] is a second entry for joint %u", who, k, d.joint);
        seen[d.joint] = 1;
        if (!(d.linear >= 0.0 && std::isfinite(d.linear)))
            return set_error(XPBD_E_INVALID, "%s: list[%u].linear = %g (must be >= 0 and finite)", who, k, d.linear);
        if (!(d.angular >= 0.0 && std::isfinite(d.angular)))
            return set_error(XPBD_E_INVALID, "%s: list[%u].angular = %g (must be >= 0 and finite)", who, k, d.angular);
    }
    return XPBD_OK;
}

int check_joint_limits(const char *who, const xpbd_joint *joints, uint32_t n_joints, const xpbd_joint_limit *limits, uint32_t n_limits)
{
    if (n_limits && !limits)
        return set_error(XPBD_E_INVALID, "%s: NULL argument", who);
    auto unit = [](const double *v) {
        const double len2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        return len2 > 0.999 && len2 < 1.001; // the hinge's tolerance (xpbd_world_set_joints)
    };
    auto perpendicular = [](const double *v, const double *axis) {
        const double d = v[0] * axis[0] + v[1] * axis[1] + v[2] * axis[2];
        return d > -1e-3 && d < 1e-3;
    };
    std::vector<uint8_t> kinds_seen(n_joints, 0);
    for (uint32_t k = 0; k < n_limits; ++k) {
        const xpbd_joint_limit &l = limits[k];
        if (l.joint >= n_joints)
            return set_error(XPBD_E_INVALID, "%s: limit %u names joint %u of %u", who, k, l.joint, n_joints);
        const xpbd_joint &j = joints[l.joint];
        if (l.kind == XPBD_LIMIT_HINGE) {
            if (j.kind != XPBD_JOINT_HINGE && j.kind != XPBD_JOINT_SLIDER)
                return set_error(XPBD_E_INVALID, "%s: limit %u is a HINGE limit on joint %u of kind %u", who, k, l.joint, j.kind);
        } else if (l.kind == XPBD_LIMIT_SLIDE) {
            if (j.kind != XPBD_JOINT_SLIDER)
                return set_error(XPBD_E_INVALID, "%s: limit %u is a SLIDE limit on joint %u of kind %u", who, k, l.joint, j.kind);
        } else if (l.kind == XPBD_LIMIT_SWING || l.kind == XPBD_LIMIT_TWIST) {
            if (j.kind != XPBD_JOINT_DISTANCE)
                return set_error(XPBD_E_INVALID, "%s: limit %u (kind %u) needs a DISTANCE joint, joint %u is of kind %u", who, k, l.kind, l.joint, j.kind);
            if (!unit(j.axis_a) || !unit(j.axis_b))
                return set_error(XPBD_E_INVALID, "%s: limit %u needs unit axes on joint %u", who, k, l.joint);
        } else {
            return set_error(XPBD_E_INVALID, "%s: limit %u has unknown kind %u", who, k, l.kind);
        }
        if (kinds_seen[l.joint] & (1u << l.kind))
            return set_error(XPBD_E_INVALID, "%s: joint %u has two limits of kind %u", who, l.joint, l.kind);
        kinds_seen[l.joint] |= (uint8_t)(1u << l.kind);
        if (l.kind == XPBD_LIMIT_SLIDE) { // metres: finite, lower <= upper; the references are not read
            if (!(l.lower <= l.upper) || !std::isfinite(l.lower) || !std::isfinite(l.upper))
                return set_error(XPBD_E_INVALID, "%s: slide limit %u has bounds [%g, %g] (need finite lower <= upper)", who, k, l.lower, l.upper);
            continue;
        }
        if (l.kind != XPBD_LIMIT_SWING) {
            if (!unit(l.ref_a) || !unit(l.ref_b))
                return set_error(XPBD_E_INVALID, "%s: limit %u needs unit references", who, k);
            if (!perpendicular(l.ref_a, j.axis_a) || !perpendicular(l.ref_b, j.axis_b))
                return set_error(XPBD_E_INVALID, "%s: limit %u: a reference is not perpendicular to its axis", who, k);
        }
        if (!(l.lower >= -M_PI && l.lower <= l.upper && l.upper <= M_PI)) // (NaN fails every comparison)
            return set_error(XPBD_E_INVALID, "%s: limit %u has bounds [%g, %g] (need -pi <= lower <= upper <= pi)", who, k, l.lower, l.upper);
        if (l.kind == XPBD_LIMIT_SWING && l.lower != 0.0)
            return set_error(XPBD_E_INVALID, "%s: swing limit %u needs lower = 0 (got %g)", who, k, l.lower);
    }
    return XPBD_OK;
}

int check_joint_drives(const char *who, const xpbd_joint *joints, uint32_t n_joints, const xpbd_joint_drive *drives, uint32_t n_drives)
{
    if (n_drives && !drives)
        return set_error(XPBD_E_INVALID, "%s: NULL argument", who);
    auto unit = [](const double *v) {
        const double len2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        return len2 > 0.999 && len2 < 1.001; // the limits' tolerances (check_joint_limits)
    };
    auto perpendicular = [](const double *v, const double *axis) {
        const double d = v[0] * axis[0] + v[1] * axis[1] + v[2] * axis[2];
        return d > -1e-3 && d < 1e-3;
    };
    std::vector<uint8_t> seen(n_joints, 0); // bit 0: an angular drive, bit 1: a linear one
    for (uint32_t k = 0; k < n_drives; ++k) {
        const xpbd_joint_drive &d = drives[k];
        if (d.joint >= n_joints)
            return set_error(XPBD_E_INVALID, "%s: drive %u names joint %u of %u", who, k, d.joint, n_joints);
        const xpbd_joint &j = joints[d.joint];
        const bool angular = d.kind == XPBD_DRIVE_ANGLE || d.kind == XPBD_DRIVE_ANGULAR_VELOCITY;
        if (!angular && d.kind != XPBD_DRIVE_POSITION && d.kind != XPBD_DRIVE_VELOCITY)
            return set_error(XPBD_E_INVALID, "%s: drive %u has unknown kind %u", who, k, d.kind);
        if (angular ? (j.kind != XPBD_JOINT_HINGE && j.kind != XPBD_JOINT_SLIDER) : j.kind != XPBD_JOINT_SLIDER)
            return set_error(XPBD_E_INVALID, "%s: drive %u (kind %u) does not fit joint %u of kind %u", who, k, d.kind, d.joint, j.kind);
        const uint8_t bit = angular ? 1u : 2u;
        if (seen[d.joint] & bit)
            return set_error(XPBD_E_INVALID, "%s: joint %u has two %s drives", who, d.joint, angular ? "angular" : "linear");
        seen[d.joint] |= bit;
        if (angular) {
            if (!unit(d.ref_a) || !unit(d.ref_b))
                return set_error(XPBD_E_INVALID, "%s: drive %u needs unit references", who, k);
            if (!perpendicular(d.ref_a, j.axis_a) || !perpendicular(d.ref_b, j.axis_b))
                return set_error(XPBD_E_INVALID, "%s: drive %u: a reference is not perpendicular to its axis", who, k);
        }
        if (!std::isfinite(d.target))
            return set_error(XPBD_E_INVALID, "%s: drive %u has target %g", who, k, d.target);
        if (d.kind == XPBD_DRIVE_ANGLE && !(d.target >= -M_PI && d.target <= M_PI))
            return set_error(XPBD_E_INVALID, "%s: angle drive %u has target %g (need -pi <= target <= pi)", who, k, d.target);
        if (!(d.compliance >= 0.0) || !std::isfinite(d.compliance))
            return set_error(XPBD_E_INVALID, "%s: drive %u has compliance %g (need finite, >= 0)", who, k, d.compliance);
        if (!(d.max_force > 0.0)) // (NaN fails the comparison; +inf passes)
            return set_error(XPBD_E_INVALID, "%s: drive %u has max_force %g (need > 0, +inf allowed)", who, k, d.max_force);
    }
    return XPBD_OK;
}

int check_edit_indices(const char *who, const uint32_t *indices, uint32_t n, uint32_t n_bodies, bool unique)
{
    if (n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (!indices) {
        if (n != n_bodies)
            return set_error(XPBD_E_INVALID, "%s: indices == NULL names the bodies 0..n-1, but n = %u and the world holds %u bodies", who, n, n_bodies);
        return XPBD_OK;
    }
    std::vector<uint8_t> seen(unique ? n_bodies : 0u, 0);
    for (uint32_t k = 0; k < n; ++k) {
        if (indices[k] >= n_bodies)
            return set_error(XPBD_E_INVALID, "%s: indices[%u] = %u but the world holds %u bodies", who, k, indices[k], n_bodies);
        if (unique && seen[indices[k]]++)
            return set_error(XPBD_E_INVALID, "%s: indices[%u] = %u is listed twice", who, k, indices[k]);
    }
    return XPBD_OK;
}

int check_edit_finite(const char *who, const char *what, const double *values, size_t count)
{
    for (size_t k = 0; values && k < count; ++k)
        if (!std::isfinite(values[k]))
            return set_error(XPBD_E_INVALID, "%s: %s[%zu] = %g (must be finite)", who, what, k, values[k]);
    return XPBD_OK;
}

int check_impulses(const char *who, const xpbd_impulse *list, uint32_t n, uint32_t n_bodies)
{
    if (!list)
        return set_error(XPBD_E_INVALID, "%s: NULL list", who);
    if (n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    for (uint32_t k = 0; k < n; ++k) {
        const xpbd_impulse &e = list[k];
        if (e.body >= n_bodies)
            return set_error(XPBD_E_INVALID, "%s: list[%u].body = %u but the world holds %u bodies", who, k, e.body, n_bodies);
        if (e.flags & ~XPBD_IMPULSE_AT_CENTRE)
            return set_error(XPBD_E_INVALID, "%s: list[%u] has unknown flags 0x%x", who, k, e.flags);
        bool finite = true;
        for (int a = 0; a < 3; ++a)
            finite = finite && std::isfinite(e.impulse[a]) && std::isfinite(e.angular_impulse[a]) &&
                     ((e.flags & XPBD_IMPULSE_AT_CENTRE) || std::isfinite(e.point[a]));
        if (!finite)
            return set_error(XPBD_E_INVALID, "%s: list[%u] has a component that is not finite", who, k);
    }
    return XPBD_OK;
}

int IslandsTarget::check(const char *who, uint32_t flags, const void *records, uint32_t cap, const void *count) const
{
    if (!count)
        return set_error(XPBD_E_INVALID, "%s: NULL count", who);
    if (!records && cap)
        return set_error(XPBD_E_INVALID, "%s: NULL records with cap = %u", who, cap);
    if (flags & ~(XPBD_ISLANDS_NO_JOINTS | XPBD_ISLANDS_NO_CONTACTS))
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x", who, flags);
    if ((flags & XPBD_ISLANDS_NO_JOINTS) && (flags & XPBD_ISLANDS_NO_CONTACTS))
        return set_error(XPBD_E_INVALID, "%s: XPBD_ISLANDS_NO_JOINTS and XPBD_ISLANDS_NO_CONTACTS together leave no edges", who);
    if (n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (flags & XPBD_ISLANDS_NO_CONTACTS)
        return XPBD_OK;
    if (!report_on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_world_set_contact_report); XPBD_ISLANDS_NO_CONTACTS needs none", who);
    if (!report_frame)
        return set_error(XPBD_E_INVALID, "%s: no report: no substep of XPBD_MODE_CONTACTS has run since the last broadphase, upload, "
                                         "history restore, enable, failed step or step in another mode", who);
    return XPBD_OK;
}

int SensorTarget::table_check(const char *who, const uint8_t *is_sensor, uint32_t n, bool get, uint32_t *count) const
{
    if (n && !is_sensor)
        return set_error(XPBD_E_INVALID, "%s: NULL is_sensor with n = %u", who, n);
    if (n != n_bodies && (get || n || is_sensor))
        return set_error(XPBD_E_INVALID, "%s: n = %u but the world holds %u bodies", who, n, n_bodies);
    uint32_t flagged = 0;
    for (uint32_t i = 0; !get && i < n; ++i) {
        if (is_sensor[i] > 1u)
            return set_error(XPBD_E_INVALID, "%s: is_sensor[%u] = %u (0 or 1: the other bits are reserved)", who, i, (unsigned)is_sensor[i]);
        flagged += is_sensor[i];
    }
    if (count)
        *count = flagged;
    return XPBD_OK;
}

int SensorTarget::overlaps_check(const char *who, const void *sensors, const void *offsets, const void *hits, uint32_t cap, const uint32_t *n_out,
                                 bool host) const
{
    if (!sensors || !offsets)
        return set_error(XPBD_E_INVALID, "%s: NULL sensors or offsets", who);
    if (!hits && cap)
        return set_error(XPBD_E_INVALID, "%s: NULL hits with cap = %u", who, cap);
    if (host && !n_out)
        return set_error(XPBD_E_INVALID, "%s: NULL n_out", who);
    if (n_sensors == 0)
        return set_error(XPBD_E_INVALID, "%s: no sensor is set (xpbd_world_set_sensors)", who);
    if (!report_on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_world_set_contact_report)", who);
    if (!report_frame)
        return set_error(XPBD_E_INVALID, "%s: no report: no substep of XPBD_MODE_CONTACTS has run since the last broadphase, upload, "
                                         "history restore, enable, failed step or step in another mode", who);
    return XPBD_OK;
}

int SleepTarget::check(const char *who, const xpbd_sleep_config &cfg) const
{
    if (!(cfg.linear_speed >= 0.0) || !std::isfinite(cfg.linear_speed))
        return set_error(XPBD_E_INVALID, "%s: linear_speed = %g (must be finite and >= 0)", who, cfg.linear_speed);
    if (!(cfg.angular_speed >= 0.0) || !std::isfinite(cfg.angular_speed))
        return set_error(XPBD_E_INVALID, "%s: angular_speed = %g (must be finite and >= 0)", who, cfg.angular_speed);
    if (cfg.frames_to_sleep == 0)
        return set_error(XPBD_E_INVALID, "%s: frames_to_sleep must be >= 1", who);
    if (cfg.flags)
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x", who, cfg.flags);
    if (mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "%s: sleeping needs XPBD_MODE_CONTACTS (world is in mode %u)", who, mode);
    if (!report_on)
        return set_error(XPBD_E_INVALID, "%s: sleeping needs the contact report (xpbd_world_set_contact_report)", who);
    return XPBD_OK;
}

int SleepTarget::state_check(const char *who) const
{
    if (!sleeping_on)
        return set_error(XPBD_E_INVALID, "%s: sleeping is off (xpbd_world_set_sleeping)", who);
    return XPBD_OK;
}

int SleepTarget::wake_check(const char *who, const uint32_t *indices, uint32_t n) const
{
    if (int rc = state_check(who))
        return rc;
    if (!indices && n)
        return set_error(XPBD_E_INVALID, "%s: NULL indices with n = %u (NULL with n == 0 wakes everybody)", who, n);
    for (uint32_t k = 0; k < n; ++k)
        if (indices[k] >= n_bodies)
            return set_error(XPBD_E_INVALID, "%s: indices[%u] = %u but the world holds %u bodies", who, k, indices[k], n_bodies);
    return XPBD_OK;
}

int JointStateTarget::check(const char *who, const uint32_t *joints, uint32_t n, const void *out, bool host) const
{
    if (n && !out)
        return set_error(XPBD_E_INVALID, "%s: NULL out with n = %u", who, n);
    if (!joints && n != n_joints)
        return set_error(XPBD_E_INVALID, "%s: joints == NULL names the joints 0..n-1, but n = %u and the world holds %u joints", who, n, n_joints);
    for (uint32_t k = 0; host && joints && k < n; ++k)
        if (joints[k] >= n_joints)
            return set_error(XPBD_E_INVALID, "%s: joints[%u] = %u but the world holds %u joints", who, k, joints[k], n_joints);
    return XPBD_OK;
}

int DriveTargets::check(const char *who, const uint32_t *drives, const double *targets, uint32_t n, bool host) const
{
    if (n && !targets)
        return set_error(XPBD_E_INVALID, "%s: NULL targets with n = %u", who, n);
    if (!drives && n != n_drives)
        return set_error(XPBD_E_INVALID, "%s: drives == NULL names the drives 0..n-1, but n = %u and the world holds %u drives", who, n, n_drives);
    for (uint32_t k = 0; host && k < n; ++k) {
        const uint32_t d = drives ? drives[k] : k;
        if (d >= n_drives)
            return set_error(XPBD_E_INVALID, "%s: drives[%u] = %u but the world holds %u drives", who, k, d, n_drives);
        if (drives && k && drives[k - 1] >= d)
            return set_error(XPBD_E_INVALID, "%s: drives[%u] = %u does not ascend from drives[%u] = %u", who, k, d, k - 1, drives[k - 1]);
        if (!std::isfinite(targets[k])) // (xpbd_world_set_joint_drives' target rules)
            return set_error(XPBD_E_INVALID, "%s: targets[%u] = %g (must be finite)", who, k, targets[k]);
        if (resident[d].kind == XPBD_DRIVE_ANGLE && !(targets[k] >= -M_PI && targets[k] <= M_PI))
            return set_error(XPBD_E_INVALID, "%s: targets[%u] = %g for angle drive %u (need -pi <= target <= pi)", who, k, targets[k], d);
    }
    return XPBD_OK;
}

namespace {
// The value rules of a kinematic entry: `row` is linear[3] followed by angular[4].
int check_kinematic_row(const char *who, const char *what, uint32_t k, uint32_t mode, const double *row)
{
    for (uint32_t c = 0; c < 7; ++c)
        if (!std::isfinite(row[c]))
            return set_error(XPBD_E_INVALID, "%s: %s[%u] has %s[%u] = %g (must be finite)", who, what, k, c < 3 ? "linear" : "angular", c < 3 ? c : c - 3,
                             row[c]);
    if (mode == XPBD_KINEMATIC_POSE && row[3] == 0.0 && row[4] == 0.0 && row[5] == 0.0 && row[6] == 0.0)
        return set_error(XPBD_E_INVALID, "%s: %s[%u] has an all-zero target rotation", who, what, k);
    return XPBD_OK;
}
} // namespace

int KinematicTarget::check(const char *who, const xpbd_kinematic *list, uint32_t n) const
{
    static_assert(sizeof(xpbd_kinematic) == 64 && offsetof(xpbd_kinematic, linear) == 8 && offsetof(xpbd_kinematic, angular) == 32,
                  "xpbd_kinematic is {body, mode, linear[3], angular[4]}: seven consecutive doubles");
    if (n && !list)
        return set_error(XPBD_E_INVALID, "%s: NULL list with n = %u", who, n);
    if (n && n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    for (uint32_t k = 0; k < n; ++k) {
        const xpbd_kinematic &e = list[k];
        if (e.body >= n_bodies)
            return set_error(XPBD_E_INVALID, "%s: list[%u].body = %u but the world holds %u bodies", who, k, e.body, n_bodies);
        if (k && list[k - 1].body >= e.body)
            return set_error(XPBD_E_INVALID, "%s: list[%u].body = %u does not ascend from list[%u].body = %u", who, k, e.body, k - 1, list[k - 1].body);
        if (e.mode != XPBD_KINEMATIC_POSE && e.mode != XPBD_KINEMATIC_VELOCITY)
            return set_error(XPBD_E_INVALID, "%s: list[%u] has unknown mode %u", who, k, e.mode);
        if (int rc = check_kinematic_row(who, "list", k, e.mode, e.linear))
            return rc;
    }
    return XPBD_OK;
}

int KinematicTarget::fixed_check(const char *who, const xpbd_kinematic *list, uint32_t n, const double *mass) const
{
    for (uint32_t k = 0; k < n; ++k)
        for (uint32_t f = 0; f < 10; ++f)
            if (!(mass[(size_t)k * 10 + f] == 0.0))
                return set_error(XPBD_E_INVALID, "%s: list[%u].body = %u is not fixed (%s = %g; a kinematic body has zero inverse mass and inertia)", who, k,
                                 list[k].body, f ? "an inverse_inertia entry" : "inverse_mass", mass[(size_t)k * 10 + f]);
    return XPBD_OK;
}

int KinematicTargets::check(const char *who, const uint32_t *entries, const double *rows, uint32_t n, bool host) const
{
    if (n && !rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows with n = %u", who, n);
    if (!entries && n != n_entries)
        return set_error(XPBD_E_INVALID, "%s: entries == NULL names the entries 0..n-1, but n = %u and the table holds %u entries", who, n, n_entries);
    if (!host && n > (1u << 29))
        return set_error(XPBD_E_INVALID, "%s: n = %u (at most 2^29 entries)", who, n);
    if (!host && (reinterpret_cast<uintptr_t>(rows) & 7u))
        return set_error(XPBD_E_INVALID, "%s: dev_rows is not 8-byte aligned", who);
    for (uint32_t k = 0; host && k < n; ++k) {
        const uint32_t e = entries ? entries[k] : k;
        if (e >= n_entries)
            return set_error(XPBD_E_INVALID, "%s: entries[%u] = %u but the table holds %u entries", who, k, e, n_entries);
        if (entries && k && entries[k - 1] >= e)
            return set_error(XPBD_E_INVALID, "%s: entries[%u] = %u does not ascend from entries[%u] = %u", who, k, e, k - 1, entries[k - 1]);
        if (int rc = check_kinematic_row(who, "rows", k, resident[e].mode, rows + (size_t)k * 7))
            return rc;
    }
    return XPBD_OK;
}

int MassEditTarget::check(const char *who, const uint32_t *indices, uint32_t n, const double *rows, uint32_t flags, bool host) const
{
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows with n = %u", who, n);
    if (n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (!mass_flags_known(flags))
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x (a layout, XPBD_MASS_INVERSE or XPBD_MASS_DIRECT, and XPBD_MASS_KEEP_FRAME)", who, flags);
    if (!host) {
        if (!indices && n != n_bodies)
            return set_error(XPBD_E_INVALID, "%s: dev_indices == NULL names the bodies 0..n-1, but n = %u and the world holds %u bodies", who, n, n_bodies);
        if (n > (1u << 29))
            return set_error(XPBD_E_INVALID, "%s: n = %u (at most 2^29 entries per call)", who, n);
        if (reinterpret_cast<uintptr_t>(rows) & 7u)
            return set_error(XPBD_E_INVALID, "%s: dev_rows is not 8-byte aligned", who);
        return XPBD_OK;
    }
    if (int rc = check_edit_indices(who, indices, n, n_bodies, true))
        return rc;
    const uint32_t layout = flags & kMassLayoutBits;
    for (uint32_t k = 0; k < n; ++k) {
        const double *row = rows + (size_t)k * kMassRowDoubles;
        double out[kMassRowDoubles];
        switch (resolve_mass_row(row, layout, out)) {
        case kMassRowOk:
            break;
        case kMassRowNotFinite:
            return set_error(XPBD_E_INVALID, "%s: rows[%u] has a value that is not finite", who, k);
        case kMassRowNegativeInverseMass:
            return set_error(XPBD_E_INVALID, "%s: rows[%u] has inverse_mass = %g (must be >= 0)", who, k, row[0]);
        case kMassRowMassNotPositive:
            return set_error(XPBD_E_INVALID, "%s: rows[%u] has mass = %g (XPBD_MASS_DIRECT needs mass > 0)", who, k, row[0]);
        case kMassRowSingular:
            return set_error(XPBD_E_SINGULAR_INERTIA, "%s: rows[%u]: the inertia tensor is not invertible (its determinant is 0)", who, k);
        }
        if (mass_row_fixed(out))
            continue;
        const uint32_t body = indices ? indices[k] : k;
        const xpbd_kinematic *end = kinematic + n_kinematic;
        const xpbd_kinematic *at = std::lower_bound(kinematic, end, body, [](const xpbd_kinematic &e, uint32_t b) { return e.body < b; });
        if (at != end && at->body == body)
            return set_error(XPBD_E_INVALID, "%s: rows[%u] gives mass to body %u, which has an entry in the kinematic table (clear it with "
                                             "xpbd_world_set_kinematics first)", who, k, body);
    }
    return XPBD_OK;
}

int MassEditTarget::get_check(const char *who, const uint32_t *indices, uint32_t n, const void *rows) const
{
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows with n = %u", who, n);
    return check_edit_indices(who, indices, n, n_bodies, false);
}

// The flags' part of the scene queries' checks: `known` are the family's own bits.
int check_query_flags(const char *who, const QueryTarget &t, uint32_t flags, uint32_t known)
{
    if (flags & ~(known | (t.terrain_allowed ? XPBD_QUERY_TERRAIN : 0u)))
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x", who, flags);
    if ((flags & XPBD_QUERY_TERRAIN) && !t.has_terrain)
        return set_error(XPBD_E_INVALID, "%s: XPBD_QUERY_TERRAIN but the world has no terrain (xpbd_world_set_terrain)", who);
    return XPBD_OK;
}

int check_raycast(const char *who, const QueryTarget &t, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, const void *hits, bool host)
{
    if (n_rays && (!rays || !hits))
        return set_error(XPBD_E_INVALID, "%s: NULL rays or hits", who);
    if (int rc = check_query_flags(who, t, flags, XPBD_RAYCAST_BRUTE_FORCE))
        return rc;
    if (!t.has_topology)
        return set_error(XPBD_E_INVALID, "%s: call %s first", who, t.setter);
    for (uint32_t r = 0; host && r < n_rays; ++r)
        if (rays[r].reserved)
            return set_error(XPBD_E_INVALID, "%s: ray %u has reserved = %u (must be 0)", who, r, rays[r].reserved);
    return XPBD_OK;
}

int check_overlap(const char *who, const QueryTarget &t, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags,
                  const void *offsets, const void *hits, uint32_t cap, const uint32_t *n_out, bool host)
{
    if (n_queries && (!queries || !offsets || (host && !n_out)))
        return set_error(XPBD_E_INVALID, "%s: NULL queries, offsets or n_out", who);
    if (cap && !hits)
        return set_error(XPBD_E_INVALID, "%s: NULL hits with cap = %u", who, cap);
    if (int rc = check_query_flags(who, t, flags, XPBD_OVERLAP_BRUTE_FORCE | XPBD_OVERLAP_MASKED))
        return rc;
    if (!t.has_topology)
        return set_error(XPBD_E_INVALID, "%s: call %s first", who, t.setter);
    for (uint32_t q = 0; host && q < n_queries; ++q) {
        if (queries[q].reserved)
            return set_error(XPBD_E_INVALID, "%s: query %u has reserved = %u (must be 0)", who, q, queries[q].reserved);
        if (queries[q].shape >= t.n_shapes)
            return set_error(XPBD_E_INVALID, "%s: query %u has shape = %u but the table holds %u shapes", who, q, queries[q].shape, t.n_shapes);
    }
    if (t.n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    return XPBD_OK;
}

int check_sweep(const char *who, const QueryTarget &t, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, const void *hits, bool host)
{
    if (n_sweeps && (!sweeps || !hits))
        return set_error(XPBD_E_INVALID, "%s: NULL sweeps or hits", who);
    if (int rc = check_query_flags(who, t, flags, XPBD_SWEEP_BRUTE_FORCE | XPBD_SWEEP_MASKED))
        return rc;
    if (!t.has_topology)
        return set_error(XPBD_E_INVALID, "%s: call %s first", who, t.setter);
    for (uint32_t q = 0; host && q < n_sweeps; ++q)
        if (sweeps[q].reserved)
            return set_error(XPBD_E_INVALID, "%s: sweep %u has reserved = %u (must be 0)", who, q, sweeps[q].reserved);
    if (t.n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    return XPBD_OK;
}

int check_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, const void *hits,
                   bool host)
{
    if (n_queries && (!queries || !hits))
        return set_error(XPBD_E_INVALID, "%s: NULL queries or hits", who);
    if (flags & ~(XPBD_DISTANCE_BRUTE_FORCE | XPBD_DISTANCE_MASKED)) // (XPBD_QUERY_TERRAIN too: the terrain is no body)
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x", who, flags);
    if (!t.has_topology)
        return set_error(XPBD_E_INVALID, "%s: call %s first", who, t.setter);
    for (uint32_t q = 0; host && q < n_queries; ++q)
        if (queries[q].reserved)
            return set_error(XPBD_E_INVALID, "%s: query %u has reserved = %u (must be 0)", who, q, queries[q].reserved);
    if (t.n_bodies == 0)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    return XPBD_OK;
}

int check_terrain_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                           const void *hits, bool host)
{
    if (n_queries && (!queries || !hits))
        return set_error(XPBD_E_INVALID, "%s: NULL queries or hits", who);
    if (flags & ~(XPBD_DISTANCE_BRUTE_FORCE | XPBD_DISTANCE_MASKED)) // (XPBD_QUERY_TERRAIN too: the call is the terrain's already)
        return set_error(XPBD_E_INVALID, "%s: unknown flags 0x%x", who, flags);
    for (uint32_t q = 0; host && q < n_queries; ++q)
        if (queries[q].reserved)
            return set_error(XPBD_E_INVALID, "%s: query %u has reserved = %u (must be 0)", who, q, queries[q].reserved);
    if (!t.has_terrain)
        return set_error(XPBD_E_INVALID, "%s: the world has no terrain (xpbd_world_set_terrain)", who);
    return XPBD_OK;
}

} // namespace xpbd
