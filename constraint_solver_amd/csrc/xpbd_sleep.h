// xpbd_sleep.h -- island SLEEPING (EXTENSION): launchers for xpbd_sleep.hip.  Semantics: include/xpbd.h, "SLEEPING".
//
// Per body: asleep, rest_frames, group (the first body of the island it fell asleep with).  Wake requests are marks on a
// group's first body; one kernel wakes every sleeper whose group is marked.  The end-of-frame pass marks from the report's
// touching pairs, wakes, counts the frames at rest, takes the minimum of the counters over every island (the islands unit's
// grouping: parent[i] = smallest member) and puts the islands that have rested long enough to sleep.  Integer atomics only
// (or, add, min), which commute: every result is independent of the schedule.
#pragma once

#include "xpbd_contacts.h"
#include "xpbd_joint_state.h"
#include "xpbd_kinematic.h"

namespace xpbd {

constexpr uint32_t kSleepCtrlWords = 64;
// ctrl[]: requests that name no group (kSleepWakeAll | kSleepZeroCounters); bodies woken / put to sleep by the last pass;
// asleep bodies and sleeping groups as launch_sleep_tally left them
enum SleepCtrl : uint32_t { SC_REQUESTS = 0, SC_WOKEN = 1, SC_SLEPT = 2, SC_ASLEEP = 3, SC_GROUPS = 4 };
constexpr uint32_t kSleepWakeAll = 1u, kSleepZeroCounters = 2u;

struct SleepState {
    // state (what the history carries)
    uint32_t *rest_frames; // [stride]
    uint32_t *group;       // [stride] XPBD_SLEEP_GROUP_NONE while awake
    uint32_t *mark;        // [stride] mark[g] != 0: group g has been asked to wake
    uint32_t *ctrl;        // [kSleepCtrlWords]
    uint8_t *asleep;       // [stride]
    // scratch of a frame
    uint8_t *fixed;        // [stride] as the islands unit defines it, from the mass properties at the start of the frame
    uint8_t *inert;        // [stride] asleep or fixed: what the broadphase reads
    uint8_t *moving;       // [stride] a MOVING kinematic body of the frame (k_kinematic_velocities; only read where a world has a table)
    uint32_t *island_min;  // [stride] by an island's first body: the smallest rest_frames of its members, 0 with a sleeper
    uint32_t n, stride;
};

// Start of a frame, before the broadphase: fixed[] from `stat`, then every sleeper wakes whose group is marked, or all of them
// under kSleepWakeAll (`requests` | ctrl[SC_REQUESTS]); kSleepZeroCounters zeroes every rest_frames; inert[] for the frame;
// marks and ctrl[SC_REQUESTS] are cleared behind it.
hipError_t launch_sleep_frame_begin(const SleepState &s, const double *stat, uint32_t requests, hipStream_t stream);
// After the broadphase: the record of every sleeper from its resting pose into both record sets (past frame = current frame =
// Rigid::frame(), pose after ground = pose); with `post` its 13 dynamic doubles there too (the restitution pass reads its
// neighbours' state after derive from it); with `trace` its contact mask into the `trace_rows` rows of the step's trace.
hipError_t launch_sleep_records(const SleepState &s, const BodyArrays &b, double *rec_a, double *rec_b, double *post, const uint32_t *last_mask,
                                uint32_t *trace, uint32_t trace_rows, hipStream_t stream);
// A MOVING kinematic body is not inert in its frame: inert[body] = 0 for every entry of `t` whose body has moving[] set (a
// fixed body is never asleep).  Behind launch_sleep_frame_begin, only in a world with a kinematic table.
hipError_t launch_sleep_moving_inert(const SleepState &s, const KinematicTable &t, hipStream_t stream);
// What the end-of-frame wake reads of the frame's MOVING bodies (default: none, the launches of a world without a table):
// moving[], the frame's pair list (not the touching set: a platform that moves away stops touching in the first substep) and the
// joints.
struct MovingBodies {
    const uint8_t *moving = nullptr; // [n]
    const uint32_t *pairs = nullptr; // [n_pairs][2]
    uint32_t n_pairs = 0;
    const Joint *joints = nullptr;
    uint32_t n_joints = 0;
};
// End of a frame: wake (marks from the `key_lanes` >= *key_count touching pairs `keys`, a << 32 | b; NULL: none), count
// (speed limits squared on the host), and, after the islands unit has grouped the frame (launch_sleep_islands below), sleep.
hipError_t launch_sleep_wake_count(const SleepState &s, const double *dyn, const unsigned long long *keys, const uint32_t *key_count,
                                   uint32_t key_lanes, double linear2, double angular2, hipStream_t stream,
                                   const MovingBodies &moving = MovingBodies());
// parent: the islands unit's flattened parents (parent[i] = first body of i's island); status: its give-up word (nonzero: nobody sleeps).
hipError_t launch_sleep_islands(const SleepState &s, double *dyn, const uint32_t *parent, const uint32_t *status, uint32_t frames_to_sleep,
                                hipStream_t stream);
// Wake requests from an index list: entry k names body indices[k * every] (indices == NULL: body k).  A sleeper's group is
// marked, a fixed body (from `stat`) sets kSleepWakeAll, an index outside the world is skipped.
hipError_t launch_sleep_request(const SleepState &s, const double *stat, const uint32_t *indices, uint32_t every, uint32_t n, hipStream_t stream);
// Wake requests of a retarget list (xpbd_world_set_drive_targets; DriveTable and the entry rules: xpbd_joint_state.h): for every
// entry the call accepts, the groups of the asleep ends of its drive's joint are marked.
hipError_t launch_sleep_request_drives(const SleepState &s, const DriveTable &t, const Joint *joints, uint32_t n_joints, const uint32_t *drives,
                                       const double *targets, uint32_t n, hipStream_t stream);
// ctrl[SC_ASLEEP], ctrl[SC_GROUPS] from the state as it stands.
hipError_t launch_sleep_tally(const SleepState &s, hipStream_t stream);

} // namespace xpbd
