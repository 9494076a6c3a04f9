// xpbd_checks.hpp -- the argument checks of the C ABI that need no device, shared by the single and the multi-GPU world (not
// installed).  Each answers XPBD_OK or XPBD_E_INVALID with a message naming `who`.  Host-only: no HIP header, builds with
// plain g++ (as xpbd_population_remap.hpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/xpbd.h"

namespace xpbd {

// The argument checks of the scene queries (the caller has dealt with a NULL world).  In order: NULL arrays, unknown flags, no
// polytopes (`setter`: the call that sets them), with `host` the records' own fields (reserved, shape: the arrays are host
// memory) and, for an overlap, a target without bodies.  A ray cast does not mind one: every ray misses.  XPBD_QUERY_TERRAIN
// is a known flag only where `terrain_allowed` (the single world; the multi-GPU world has no terrain), and then needs
// `has_terrain`: without one the call is refused right after the flags, naming xpbd_world_set_terrain, as
// xpbd_world_sample_terrain is.
struct QueryTarget {
    bool has_topology;
    uint32_t n_bodies, n_shapes;
    const char *setter;
    bool terrain_allowed = false, has_terrain = false;
};
// The flags' part of the scene queries' checks: `known` are the family's own bits.
int check_query_flags(const char *who, const QueryTarget &t, uint32_t flags, uint32_t known);
int check_raycast(const char *who, const QueryTarget &t, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, const void *hits, bool host);
// n_out: what a host variant reports its total through (NULL passes for a device variant, which has none).
int check_overlap(const char *who, const QueryTarget &t, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags,
                  const void *offsets, const void *hits, uint32_t cap, const uint32_t *n_out, bool host);
// As check_overlap; a sweep's shape is not an error, it hits nothing.
int check_sweep(const char *who, const QueryTarget &t, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, const void *hits, bool host);
// As check_sweep: NULL arrays, unknown flags, no polytopes, with `host` a nonzero `reserved`, a target without bodies.  A shape
// outside the table (XPBD_DISTANCE_POINT aside) is no error, the query finds nothing; XPBD_QUERY_TERRAIN is an unknown flag whatever
// the target (the terrain is no body).
int check_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, const void *hits,
                   bool host);
// The terrain distance queries: NULL arrays, unknown flags (everything but XPBD_DISTANCE_BRUTE_FORCE and XPBD_DISTANCE_MASKED,
// XPBD_QUERY_TERRAIN included), with `host` a nonzero `reserved`, a target without a terrain.  Neither polytopes nor bodies are
// required: without polytopes only point queries find anything.
int check_terrain_distance(const char *who, const QueryTarget &t, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags,
                           const void *hits, bool host);
// The argument checks of xpbd_world_set_joints against a world of n_bodies bodies / of xpbd_world_set_joint_limits against a
// joint list.
int check_joints(const char *who, const xpbd_joint *joints, uint32_t n_joints, uint32_t n_bodies);
int check_joint_limits(const char *who, const xpbd_joint *joints, uint32_t n_joints, const xpbd_joint_limit *limits, uint32_t n_limits);
// ... of xpbd_world_set_joint_drives against a joint list.
int check_joint_drives(const char *who, const xpbd_joint *joints, uint32_t n_joints, const xpbd_joint_drive *drives, uint32_t n_drives);
// ... of a per-body array (`what`) handed to a world of n_bodies bodies: NULL only with n == 0 (the default), else n == n_bodies.
// `count`: what the caller's interface calls n.
int check_per_body(const char *who, const char *what, const void *values, uint32_t n, uint32_t n_bodies, const char *count = "n");
// ... and of the records of xpbd_world_set_materials: friction >= 0 (+inf allowed, NaN not), reserved == 0.
int check_materials(const char *who, const xpbd_material *materials, uint32_t n);
// ... of the host variants of the body edits (include/xpbd.h, "Body EDITS") against a world of n_bodies bodies, after the
// caller has dealt with a NULL world and n == 0: a world without bodies, an index list (NULL: bodies 0..n-1, then n ==
// n_bodies; an index >= n_bodies; with `unique`, an index twice), `count` doubles that must all be finite (`what` names them;
// NULL values pass), and an impulse list (NULL, a body >= n_bodies, unknown flags, non-finite components).
int check_edit_indices(const char *who, const uint32_t *indices, uint32_t n, uint32_t n_bodies, bool unique);
int check_edit_finite(const char *who, const char *what, const double *values, size_t count);
int check_impulses(const char *who, const xpbd_impulse *list, uint32_t n, uint32_t n_bodies);
// ... of xpbd_world_islands and _islands_device (include/xpbd.h, "Contact ISLANDS"), after the caller has dealt with a NULL
// world: what the call is made on, and its check -- a NULL count, a NULL record buffer with a nonzero cap, unknown flags, both
// flags, a world without bodies, and, without XPBD_ISLANDS_NO_CONTACTS, a report that xpbd_world_contact_report_counts would
// refuse (reporting off; no frame).
// ... of the damping calls (include/xpbd.h, "DAMPING"), after the caller has dealt with a NULL world and the world's mode: what
// the call is made on, and its checks.  rows, of xpbd_world_set_damping: check_per_body's rules, then a drag coefficient that is
// negative, NaN or infinite, a cap that is <= 0 or NaN (+inf allowed); any_set (NULL: not wanted): does a row differ from the
// default {0, 0, +inf, +inf}?  dampers, of xpbd_world_set_joint_damping: a NULL list with n > 0, a joint index out of range, two
// entries for one joint, a nonzero `reserved`, a coefficient that is negative, NaN or infinite.
struct DampingTarget {
    uint32_t n_bodies, n_joints;
    int rows(const char *who, const xpbd_body_damping *rows, uint32_t n, bool *any_set = nullptr) const;
    int dampers(const char *who, const xpbd_joint_damping *list, uint32_t n) const;
};
struct IslandsTarget {
    uint32_t n_bodies;
    bool report_on, report_frame;
    int check(const char *who, uint32_t flags, const void *records, uint32_t cap, const void *count) const;
};
// ... of the sleeping calls (include/xpbd.h, "SLEEPING"), after the caller has dealt with a NULL world: what the call is made
// on.  check: xpbd_world_set_sleeping with a configuration (a negative or non-finite speed, frames_to_sleep == 0, flags, a
// mode other than XPBD_MODE_CONTACTS, the contact report off).  state_check: the state and wake calls (sleeping off).
// wake_check: the host variant's index list on top of it (NULL with n != 0, an index >= n_bodies).
struct SleepTarget {
    uint32_t mode, n_bodies;
    bool report_on, sleeping_on;
    int check(const char *who, const xpbd_sleep_config &cfg) const;
    int state_check(const char *who) const;
    int wake_check(const char *who, const uint32_t *indices, uint32_t n) const;
};

// ... of the joint states and drive targets (include/xpbd.h, "Joint STATES and drive TARGETS"), after the caller has dealt with a
// NULL world: what the call is made on.  JointStateTarget::check, of xpbd_world_joint_states(_device): a NULL out with n > 0,
// joints == NULL with n != n_joints, and with `host` (the list is host memory) an index out of range.  DriveTargets::check, of
// xpbd_world_set_drive_targets(_device) against the resident drives (`resident` is read only with `host`): NULL targets with
// n > 0, drives == NULL with n != n_drives, and with `host` an index out of range or not above its predecessor, a non-finite
// target, an ANGLE target outside [-pi, pi].
struct JointStateTarget {
    uint32_t n_joints;
    int check(const char *who, const uint32_t *joints, uint32_t n, const void *out, bool host) const;
};
struct DriveTargets {
    const xpbd_joint_drive *resident;
    uint32_t n_drives;
    int check(const char *who, const uint32_t *drives, const double *targets, uint32_t n, bool host) const;
};

// ... of the kinematic table and its targets (include/xpbd.h, "KINEMATIC bodies"), after the caller has dealt with a NULL world:
// what the call is made on.  KinematicTarget::check, of xpbd_world_set_kinematics (its check_kinematics): a NULL list with n > 0,
// no resident bodies, a body out of range or not above its predecessor, an unknown mode, a non-finite value, an all-zero POSE
// rotation; fixed_check, once the ten mass doubles of the named bodies are on the host (mass: [n][10]): a body that is not fixed.
// KinematicTargets::check, of xpbd_world_set_kinematic_targets(_device) against the resident table (its check_kinematic_targets;
// `resident` is read only with `host`): NULL rows with n > 0, entries == NULL with n != n_entries, a device list of more than
// 2^29 entries or rows that are not 8-byte aligned, and with `host` an index out of range or not above its predecessor, a
// non-finite value, an all-zero POSE rotation.
struct KinematicTarget {
    uint32_t n_bodies;
    int check(const char *who, const xpbd_kinematic *list, uint32_t n) const;
    int fixed_check(const char *who, const xpbd_kinematic *list, uint32_t n, const double *mass) const;
};
struct KinematicTargets {
    const xpbd_kinematic *resident;
    uint32_t n_entries;
    int check(const char *who, const uint32_t *entries, const double *rows, uint32_t n, bool host) const;
};

// ... of the sensor calls (include/xpbd.h, "SENSOR bodies"), after the caller has dealt with a NULL world: what the call is made
// on.  table_check, of xpbd_world_set_sensors and (get == true) _get_sensors: NULL with n > 0, n different from the body count
// (only NULL with n == 0, which clears, passes a setter without it; a getter takes no such exception), and for the setter a byte
// other than 0 or 1; count (NULL: not wanted): the bytes that are 1.  overlaps_check, of xpbd_world_sensor_overlaps(_device): a
// NULL sensors or offsets array, a NULL hits array with a nonzero cap, with `host` a NULL n_out, no sensor set, and a report that
// xpbd_world_contact_report_counts would refuse (reporting off; no frame).
struct SensorTarget {
    uint32_t n_bodies, n_sensors;
    bool report_on, report_frame;
    int table_check(const char *who, const uint8_t *is_sensor, uint32_t n, bool get, uint32_t *count = nullptr) const;
    int overlaps_check(const char *who, const void *sensors, const void *offsets, const void *hits, uint32_t cap, const uint32_t *n_out, bool host) const;
};

// ... of the mass edits (include/xpbd.h, "MASS properties of resident bodies"), after the caller has dealt with a NULL world and
// n == 0: what the call is made on -- the body count and the host copy of the kinematic table (ascending by body; read only
// with `host`).  check, of xpbd_world_set_mass_properties(_device): NULL rows, no resident bodies, unknown flag bits or a layout
// other than XPBD_MASS_INVERSE / _DIRECT; for the device variant indices == NULL with n != n_bodies, more than 2^29 entries,
// rows that are not 8-byte aligned; with `host` the index list (out of range, twice) and every row by the rules of
// resolve_mass_row (xpbd_mass_row.hpp: a non-finite value, inverse_mass < 0, DIRECT with mass <= 0; a singular DIRECT tensor is
// XPBD_E_SINGULAR_INERTIA) and the kinematic rule: a body with an entry in the table takes only a row that leaves it fixed.
// get_check, of xpbd_world_get_mass_properties: NULL rows, no resident bodies, the index list (an index may repeat).
struct MassEditTarget {
    uint32_t n_bodies;
    const xpbd_kinematic *kinematic;
    uint32_t n_kinematic;
    int check(const char *who, const uint32_t *indices, uint32_t n, const double *rows, uint32_t flags, bool host) const;
    int get_check(const char *who, const uint32_t *indices, uint32_t n, const void *rows) const;
};

} // namespace xpbd
