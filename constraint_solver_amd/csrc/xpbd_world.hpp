// xpbd_world.hpp -- the single-GPU world behind the C ABI: its state, the owners of the parts that have an invariant, and
// what the units that implement it share (not installed; no .hip file includes it).
//
//   xpbd_world.cpp           create/destroy, upload/download, the body-indexed setters, joint staging, history, step
//   xpbd_world_shapes.cpp    ShapeTables: the two shape setters and their one staged install
//   xpbd_world_contacts.cpp  Broadphase, NarrowphaseSchedule, the contact schedules and their settings, the one-shot narrowphases,
//                            the halo pieces, the frame snapshot
//   xpbd_world_report.cpp    ContactReport and the report entry points
//   xpbd_world_query.cpp     the scene-query host layer and entry points
//   xpbd_world_edit.cpp      body edits, mass edits, population changes, re-packing a shard
//   xpbd_world_islands.cpp   Islands and the island entry points
//   xpbd_world_sleep.cpp     Sleep and the sleeping entry points
//   xpbd_world_joint_state.cpp  joint states and drive targets: the entry points, and the way back of device-set targets
//   xpbd_world_kinematic.cpp    KinematicBodies and the kinematic entry points
//   xpbd_world_sensors.cpp      Sensors, the sensor entry points and what the frame, the islands and the sleep pass ask of them
#pragma once

#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "xpbd_internal.h"
#include "xpbd_kernels.h"
#include "xpbd_contacts.h"
#include "xpbd_damping.h"
#include "xpbd_gjk.h"
#include "xpbd_islands.h"
#include "xpbd_joint_state.h"
#include "xpbd_kinematic.h"
#include "xpbd_pairs.h"
#include "xpbd_population_remap.hpp"
#include "xpbd_query.h"
#include "xpbd_report.h"
#include "xpbd_sensors.h"
#include "xpbd_sleep.h"

struct xpbd_world;

// Everything here but xpbd_world itself stays inside the library: the units share it, nobody outside links to it.
#pragma GCC visibility push(hidden)

using xpbd::DeviceBuffer;
using xpbd::set_error;

constexpr uint32_t kMaxBodies = 0xFFFFFF00u; // the largest count whose stride fits 32 bits
// Sizes a buffer that must hold at least one element.
template <class T> constexpr T at_least_one(T n) { return n ? n : 1; }
inline uint32_t stride_for(uint32_t n_bodies) { return (at_least_one(n_bodies) + 255u) / 256u * 256u; }
inline uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v)
        p <<= 1;
    return p;
}

// The joints of a world: what the caller handed to xpbd_world_set_joints, _set_joint_limits, _set_joint_drives and
// _set_joint_damping, and the device tables built from it in four parts, one per setter.  A part is complete or empty (count 0,
// no buffers); only stage_csr, stage_limits, stage_extras and stage_joint_damping fill one, aside, and a setter or a population
// change moves it in.
struct JointTables {
    xpbd::JointSet set;                         // joints, limits of all kinds, drives and dampers, the caller's order (the last three
                                                // name joints by index: new joints drop them; a population change re-indexes all four)
    std::vector<xpbd_joint_limit> slide_limits; // the XPBD_LIMIT_SLIDE ones among set.limits
    struct Csr { // the joints and the CSR body -> joints
        uint32_t n = 0;
        DeviceBuffer joints, off, list;
    } csr;
    struct Limits { // the ANGULAR limits behind a CSR joint -> limits, the table the pair solve walks
        uint32_t n_limits = 0;
        DeviceBuffer limits, limit_off;
    } limits;
    struct Extras { // the lanes of k_joint_extras: the joints with extra entries (sliders, SLIDE limits, drives), the per-end sums
        uint32_t n_extra_joints = 0;
        DeviceBuffer sums, joints, slots, off, items;
        // for the joint states and drive targets: joint -> its lane here (xpbd::kNoExtraSlot: none), drive -> its item, and that
        // map on the host.  targets_on_device: xpbd_world_set_drive_targets_device has written targets that set.drives does
        // not hold yet (sync_drive_targets brings them back before anything re-stages this part from the host copy; a fresh
        // part starts clean, which is how the setters that replace the drives clear it)
        DeviceBuffer joint_slot, drive_item;
        std::vector<uint32_t> drive_item_host;
        bool targets_on_device = false;
    } extras;
    struct Damping { // (mu_l, mu_a) of every joint for stage 7 (xpbd_damping.h); empty unless a listed coefficient is nonzero
        uint32_t n = 0;
        DeviceBuffer table;
    } damping;

    void fill(xpbd::ContactBuffers &c) const // (an empty part holds no buffer: NULL)
    {
        c.joints = csr.joints.as<xpbd::Joint>();
        c.joint_off = csr.off.as<uint32_t>();
        c.joint_list = csr.list.as<uint32_t>();
        c.limits = limits.limits.as<xpbd::JointLimit>();
        c.limit_off = limits.limit_off.as<uint32_t>();
        c.joint_extra = extras.sums.as<double>();
        c.extra_joints = extras.joints.as<uint32_t>();
        c.extra_slots = extras.slots.as<uint32_t>();
        c.extra_off = extras.off.as<uint32_t>();
        c.extra_items = extras.items.as<xpbd::JointExtraItem>();
        c.n_extra_joints = extras.n_extra_joints;
    }
    xpbd::JointStateTables state_tables() const
    {
        return xpbd::JointStateTables{csr.joints.as<xpbd::Joint>(), csr.n, limits.limits.as<xpbd::JointLimit>(), limits.limit_off.as<uint32_t>(),
                                      extras.joint_slot.as<uint32_t>(), extras.off.as<uint32_t>(), extras.items.as<xpbd::JointExtraItem>()};
    }
    xpbd::DriveTable drive_table() const
    {
        return xpbd::DriveTable{extras.items.as<xpbd::JointExtraItem>(), extras.drive_item.as<uint32_t>(), (uint32_t)extras.drive_item_host.size()};
    }
    void clear() { *this = JointTables{}; }
};

// The shape tables of a world (xpbd_world_set_shapes, _set_polytopes; xpbd_shape_tables.hpp; xpbd_world_shapes.cpp), which every
// kernel reads.  The vertex part (verts, vert_offsets) and the topology part (the ten other tables, the maxima, has_topology) are
// each complete or absent, and they always describe the same n_shapes shapes.  Only stage_shape_tables fills one, aside, and only
// install_shape_tables (the two setters; the multi-GPU world for its shards) moves one in, once nothing can fail any more: a
// vertex-only set leaves no topology behind.  (Vertices alone that fit the present blocks are filled into those, with both parts
// marked absent meanwhile.)
struct ShapeTables : xpbd::ShapeCounts {
    DeviceBuffer verts, vert_offsets;
    DeviceBuffer planes, centroids, desc, face_start, face_verts, edges, radii, edge_dirs, edge_dir_id, shape_class;

    xpbd::ShapeTable shapes() const { return xpbd::ShapeTable{verts.as<double>(), vert_offsets.as<uint32_t>(), n_shapes, total_verts}; }
    xpbd::PolytopeTables tables() const
    {
        return xpbd::PolytopeTables{verts.as<double>(), planes.as<double>(), centroids.as<double>(), desc.as<xpbd::ShapeDesc>(),
                                    face_start.as<uint32_t>(), face_verts.as<uint32_t>(), edges.as<uint32_t>(), radii.as<double>(),
                                    edge_dirs.as<double>(), edge_dir_id.as<uint32_t>(), n_shapes, total_verts, max_verts, max_faces, max_face_verts,
                                    shape_class.as<uint8_t>(), two_classes, small_max_face_verts};
    }
    void clear() { *this = ShapeTables{}; }
};

// The kinematic table of a world (xpbd_world_set_kinematics; xpbd_kinematic.h; xpbd_world_kinematic.cpp): what the caller handed
// over, and its copy on the device, complete or absent (an empty table holds no block).  Only the setter and a population
// change replace the block, each staged aside and moved in once nothing can fail.  targets_on_device:
// xpbd_world_set_kinematic_targets_device has written rows that `list` does not hold yet (sync_kinematic_targets brings them
// back before a population change re-stages the table from the host copy; a fresh table starts clean).
struct KinematicBodies {
    std::vector<xpbd_kinematic> list;
    DeviceBuffer table;
    bool targets_on_device = false;

    bool any() const { return !list.empty(); }
    xpbd::KinematicTable view() const { return xpbd::KinematicTable{table.as<xpbd_kinematic>(), (uint32_t)list.size()}; }
    void clear() { *this = KinematicBodies{}; }
};

// The sensor table of a world (xpbd_world_set_sensors; xpbd_sensors.h; xpbd_world_sensors.cpp): one byte per body, what the caller
// handed over (`host`) and its copy on the device, complete or absent; `count`: the bodies flagged.  Only the setter and a
// population change replace the table, each staged aside and moved in once nothing can fail.  Everything a frame does for sensors
// hangs on any(): an empty or all-zero table enqueues nothing.  The other blocks are scratch: the masked pair codes of the
// substep under way, the report's keys without the sensor pairs, the ascending sensor list (list_ready: it describes `flags`)
// and the staging of the host variant of the occupancy.
struct Sensors {
    std::vector<uint8_t> host;
    uint32_t count = 0;
    bool list_ready = false;
    DeviceBuffer flags;
    DeviceBuffer solve_codes;
    DeviceBuffer key_flag, key_scan, solid_keys;
    DeviceBuffer list, list_flag, occ_scan, occ_sensors, occ_offsets, occ_hits;

    bool any() const { return count != 0; }
    void clear() { *this = Sensors{}; }
};

// The sphere broadphase of the contact pipeline (xpbd_world_contacts.cpp): grid, buckets, the neighbour lists and the pair
// list of the current frame with its per-pair results.  have_neighbours: the lists describe the bodies as they are.
struct Broadphase {
    DeviceBuffer centers, radius, cell, key, maxr, grid_partials, bucket_start, bucket_cursor, items, items_unsorted, slot_sphere,
        slot_cell, slot_filter, slot_inert, nbr_off, pair_first, upper_start, nbr, nbr_pair, pairs, manifolds, pair_codes, scan;
    uint32_t table_size = 0, n_entries = 0, n_pairs = 0;
    bool have_neighbours = false;
    // The broadphase in two halves (build_neighbours_enqueue / _collect): the counting kernels leave the totals the host
    // needs to size the pair buffers in PINNED memory and record an event; only the second half waits for it.  A host that
    // drives several worlds (xpbd_multi.cpp: one per GPU) enqueues all of them before it waits for any.
    struct Totals {
        uint32_t entries, pairs;
        unsigned long long stats[2];
    };
    Totals *totals = nullptr; // hipHostMalloc
    hipEvent_t event = nullptr;
    bool pending = false;

    Broadphase() = default;
    Broadphase(const Broadphase &) = delete;
    Broadphase &operator=(const Broadphase &) = delete;
    ~Broadphase() { release_host(); }
    void release_host() noexcept // the pinned block and the event (the device is bound, nothing queued uses them)
    {
        if (totals)
            (void)hipHostFree(totals);
        if (event)
            (void)hipEventDestroy(event);
        totals = nullptr;
        event = nullptr;
    }
    void fill(xpbd::ContactBuffers &c) const
    {
        c.centers = centers.as<double>();
        c.radius = radius.as<double>();
        c.cell = cell.as<int32_t>();
        c.key = key.as<uint32_t>();
        c.grid = maxr.as<xpbd::GridInfo>();
        c.grid_partials = grid_partials.as<double>();
        c.bucket_start = bucket_start.as<uint32_t>();
        c.bucket_cursor = bucket_cursor.as<uint32_t>();
        c.items = items.as<uint32_t>();
        c.items_unsorted = items_unsorted.as<uint32_t>();
        c.table_size = table_size;
        c.slot_sphere = slot_sphere.as<double>();
        c.slot_cell = slot_cell.as<int32_t>();
        c.nbr_off = nbr_off.as<uint32_t>();
        c.pair_first = pair_first.as<uint32_t>();
        c.upper_start = upper_start.as<uint32_t>();
        c.nbr = nbr.as<uint32_t>();
        c.nbr_pair = nbr_pair.as<uint32_t>();
        c.pairs = pairs.as<uint32_t>();
        c.manifolds = manifolds.as<xpbd::ContactManifold>();
        c.pair_codes = pair_codes.as<uint8_t>();
        c.scan_scratch = scan.as<uint32_t>();
    }
};

// Which narrowphase schedule the coming frame runs, and the scratch of both narrowphases (xpbd_world_contacts.cpp).
// SAT in two passes (pre-test pass + survivor list, xpbd_pairs.h): chosen per frame from the share of touching pairs in the
// previous frame, read back at the broadphase's synchronisation point.
struct NarrowphaseSchedule {
    DeviceBuffer stats; // two counters of the contact kernels: touching pairs, and what xpbd_world_contact_stats reports beside them
    DeviceBuffer sat_counters, sat_survivors, sat_axis_cache, gjk_axis_cache;
    xpbd::SatScratch sat_scratch{nullptr, nullptr, 0, nullptr, true};
    bool sat_two_pass = false;
    uint32_t sat_schedule = XPBD_SAT_SCHEDULE_AUTO;
    unsigned long long stats_touching_seen = 0, stats_pair_substeps = 0, stats_pair_substeps_seen = 0;
    DeviceBuffer gjk_counters, gjk_pairs_scratch; // hit list of the two-kernel GJK/EPA narrowphase (xpbd_gjk.h)
    xpbd::GjkScratch gjk_scratch{nullptr, nullptr, 0, nullptr, nullptr};

    // The schedule of the coming frame from the touching-pair counter as the broadphase read it back.
    void choose(unsigned long long touching_now, uint32_t two_classes);
    // Scratch of launch_gjk_epa_pairs for `n_pairs` pairs (growing it frees the old block, which waits for the device).
    int ensure_gjk_scratch(uint32_t n_pairs, hipStream_t stream);
};

// Contact reports (xpbd_world_set_contact_report; xpbd_report.h; xpbd_world_report.cpp).  keys[cur] holds this frame's
// touching pairs once compacted, keys[cur ^ 1] those of the previous frame (S_prev, when prev_valid).  Nothing starts a
// frame, no touch count, no scan runs while reporting is off.  The operations read the pair list and the stream of the world
// `w` they belong to.
struct ContactReport {
    bool on = false;
    bool frame = false;      // the current pair list counts its touching substeps in `touch` (zeroed by its broadphase)
    bool keys_ready = false; // keys[cur] is up to date with the substeps run (its count on its way to `host`)
    bool ready = false;      // `counts` and the scans behind them are up to date
    bool prev_valid = false;
    uint32_t substeps = 0, cur = 0;
    uint32_t counts[4] = {0, 0, 0, 0}; // pairs, points, begins, ends
    uint32_t *host = nullptr;          // hipHostMalloc: [0..1] key counts of keys[0..1], [2..4] point / BEGIN / event totals
    DeviceBuffer touch, flag, sel, npts, keys[2], scan, ev_flag, pairs, points, events;
    // a shard of the multi-GPU world, while a ShardLoan lives: owned slots and global ids (ReportFrame)
    const uint8_t *map_owned = nullptr;
    const uint32_t *map_ids = nullptr;

    ContactReport() = default;
    ContactReport(const ContactReport &) = delete;
    ContactReport &operator=(const ContactReport &) = delete;
    ~ContactReport() { release_host(); }
    void release_host() noexcept
    {
        if (host)
            (void)hipHostFree(host);
        host = nullptr;
    }

    void reset()
    {
        frame = keys_ready = ready = prev_valid = false;
        substeps = 0;
    }
    void release_buffers()
    {
        for (DeviceBuffer *b : {&touch, &flag, &sel, &npts, &keys[0], &keys[1], &scan, &ev_flag, &pairs, &points, &events})
            b->release();
    }
    xpbd::ReportFrame frame_of(const Broadphase &bp) const
    {
        return xpbd::ReportFrame{bp.pairs.as<uint32_t>(), bp.pair_codes.as<uint8_t>(), bp.manifolds.as<xpbd::ContactManifold>(),
                                 touch.as<uint32_t>(), bp.n_pairs, map_owned, map_ids};
    }
    int compact_keys(const xpbd_world *w);
    int frame_end(const xpbd_world *w);
    int frame_begin(const xpbd_world *w);
    int note_substep(const xpbd_world *w, const uint8_t *pair_codes);
    int prepare(const xpbd_world *w, const char *who);

    // Lends the mapping of a shard for the duration of xpbd::report_shard: the keys are compacted again with it, and once
    // more without it should the shard's world itself be asked.
    struct ShardLoan {
        ContactReport &r;
        ShardLoan(ContactReport &report, const uint8_t *owned, const uint32_t *ids) : r(report)
        {
            r.map_owned = owned;
            r.map_ids = ids;
            r.keys_ready = r.ready = false;
        }
        ~ShardLoan()
        {
            r.map_owned = nullptr;
            r.map_ids = nullptr;
            r.keys_ready = r.ready = false;
        }
    };
};

// Staging and scratch of single calls: plain aggregates (what each is for: at its member in xpbd_world).
struct ReplanStaging {
    DeviceBuffer aos, shape, src, incoming, keys, records;
};
struct FrameSnapshot {
    DeviceBuffer state;
    bool valid = false, stepped = false;
};
struct TerrainStaging {
    DeviceBuffer xy, out;
};
struct NarrowphaseStaging {
    DeviceBuffer pairs, results;
};
struct EditStaging {
    DeviceBuffer indices, values, list;
    DeviceBuffer owner; // xpbd_world_set_mass_properties_device: one claim word per body (xpbd_mass_edit.h)
};
struct PopulationScratch {
    DeviceBuffer remove, indices, prefix, scan, map, src;
};
struct History {
    DeviceBuffer states;
    uint32_t length = 0;
    std::vector<uint8_t> stepped;
    std::vector<uint8_t> sleep_requests; // Sleep::requests as they stood at the push (all 0 with sleeping off)
};

// Contact islands (xpbd_world_islands*; xpbd_islands.h; xpbd_world_islands.cpp): the scratch of one call, reserved like the
// report's -- sized by the body count, grown only when it has grown.  result: the give-up word and the island count of the
// last call, next to each other; records: what the host variant downloads from.  The operations read the bodies, the joints,
// the report and the stream of the world `w` they belong to.
struct Islands {
    DeviceBuffer parent, fixed, flag, scan, result, island_of, records;

    int reserve(const xpbd_world *w, bool host_island_of, uint32_t host_records);
    int enqueue(xpbd_world *w, uint32_t flags, uint32_t *dev_island_of, xpbd_island *dev_records, uint32_t cap, uint32_t *dev_total);
};

// Island sleeping (xpbd_world_set_sleeping; xpbd_sleep.h; xpbd_world_sleep.cpp).  `state` is what a history entry carries
// beside the bodies: rest_frames, group, the wake marks, the control words and the asleep bytes, in one block so that a push or
// a restore is one copy.  `scratch` holds what a frame derives from it.  Both follow the stride; `fresh` (after an enable, an
// upload or a population change) has ensure() start every body awake with zero counters.  requests: the wake requests made on
// the host since the last frame began that name no group (kSleepWakeAll, kSleepZeroCounters).  The operations read the bodies,
// the report, the joints and the stream of the world `w` they belong to; a world with sleeping off calls none of them.
struct Sleep {
    bool on = false, fresh = true;
    bool moving = false; // the scratch's moving[] describes the frame under way: step_contacts filled it from a non-empty kinematic table
    xpbd_sleep_config cfg{};
    uint32_t requests = 0;
    DeviceBuffer state, scratch;

    static size_t state_bytes(uint32_t stride) { return (size_t)stride * 13 + xpbd::kSleepCtrlWords * 4; }
    xpbd::SleepState view(const xpbd_world *w) const;
    const uint8_t *asleep(const xpbd_world *w) const { return view(w).asleep; }
    void wake_all(bool zero_counters)
    {
        if (on)
            requests |= xpbd::kSleepWakeAll | (zero_counters ? xpbd::kSleepZeroCounters : 0u);
    }
    int ensure(const xpbd_world *w);
    int frame_begin(xpbd_world *w);                                        // before the broadphase: the wake requests
    int frame_records(xpbd_world *w, uint32_t *trace, uint32_t trace_rows); // after it: the sleepers' records
    int frame_end(xpbd_world *w);                                          // after the last substep: the sleep pass
    // wake requests of an edit: entry k names body dev_indices[k * every] (NULL: body k)
    int request(xpbd_world *w, const uint32_t *dev_indices, uint32_t every, uint32_t n);
    // wake requests of a retarget list (xpbd_world_set_drive_targets): the asleep ends of the joints of its valid entries
    int request_drives(xpbd_world *w, const uint32_t *dev_drives, const double *dev_targets, uint32_t n);
};

#pragma GCC visibility pop

struct xpbd_world {
    int device = 0;
    uint32_t mode = XPBD_MODE_FUSED;
    uint32_t flags = 0;
    uint32_t block_size = 0;

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // bodies
    uint32_t n = 0;
    uint32_t stride = 0;
    uint32_t max_shape_id = 0; // largest shape id among the uploaded bodies (install_shape_tables re-validates against it)
    DeviceBuffer dyn, stat, shape_id, aos_staging, last_mask, trace, block_counts, contacts;
    uint32_t trace_rows = 0; // substeps recorded by the last step()
    bool stepped = false;

    // shapes: vertices, and the polytope topology for the body-body narrowphase (extension)
    ShapeTables geom;

    // extension: contact pipeline (XPBD_MODE_CONTACTS)
    double contact_pad = 0.02;
    double max_depenetration_speed = 0.0; // 0 = off (the reference's solver loop)
    uint32_t narrowphase = XPBD_NARROWPHASE_SAT;
    // the per-substep body records, and a second set for the fused "end of substep k + start of substep k + 1" kernel (step_contacts)
    DeviceBuffer dyn_alt, cb_rec, cb_rec_b, cb_stat_rec, cb_stat_shape;
    bool stat_rec_valid = false; // the StatRecords mirror the SoA static fields of the bodies uploaded last
    // Mass properties shared per shape: when every body of a shape has bit-identical inverse mass, inverse inertia and
    // centre of mass (checked on the host at upload -- the usual case: bodies are instances of a few shapes), the contact
    // kernels read them from a table of n_shapes StatRecords indexed by shape id (cache resident) instead of gathering a
    // 128-byte record per body and per neighbour.  Same values, so the same bits.
    bool stat_shared = false;
    std::vector<double> stat_shape_host; // [n_shapes][kStatRecDoubles]
    std::vector<uint8_t> stat_shape_seen; // [n_shapes] a body of the shape has been uploaded: its row of stat_shape_host is set
    Broadphase bp;
    NarrowphaseSchedule np;
    // the one-shot narrowphases (xpbd_world_narrowphase, _edge_axes_separation, _narrowphase_gjk): the caller's pairs and their results
    NarrowphaseStaging np_staging;
    ContactReport report;
    // re-planning a shard on the device (xpbd::repack_bodies, download_records, halo_cell_keys): the new world in AoS, its
    // shape ids, the source map, incoming records; the cell keys and the gathered records
    ReplanStaging replan;
    // state at the start of a frame (xpbd::frame_snapshot_save / _restore): the 13 dynamic fields and the contact masks
    FrameSnapshot snapshot;
    // Body-indexed settings: each names bodies (or the joints between them) by index, so a new set of bodies clears all seven
    // (adopt_body_count).  Values whose clear() restores the defaults; the per-body device tables stay allocated beside theirs.
    JointTables joints;
    struct Filters { // xpbd_world_set_collision_filters: group, mask per body (on), XPBD_FILTER_* flags
        bool on = false;
        uint32_t flags = 0;
        void clear() { *this = Filters{}; }
    } filters;
    DeviceBuffer ft_filters;
    // xpbd_world_set_materials: the friction coefficient of every body (on: one of them, or the ground's, has been set -- the
    // contact kernels then run their MATERIALS forms) and of the ground plane
    struct Materials {
        bool on = false;
        double ground_friction = std::numeric_limits<double>::infinity();
        void clear() { *this = Materials{}; }
    } materials;
    DeviceBuffer mt_friction;
    // xpbd_world_set_restitution: the coefficient of every body and of the ground (on: one of them is > 0 -- the step then runs
    // the unfused schedule with the velocity pass after derive; all zero runs what ran before), the start-of-substep velocities
    // the pass reads ([6][stride]); dyn_alt holds the state after derive meanwhile
    struct Restitution {
        bool on = false;
        double ground = 0.0, bounce_threshold = 0.0;
        void clear() { *this = Restitution{}; }
    } restitution;
    DeviceBuffer rs_restitution, rs_start;
    // xpbd_world_set_damping: the rows of every body, SoA ([4][at_least_one(n)]: xpbd_damping.h).  on: a row differs from the
    // default -- the step then runs the unfused schedule with stage 7 behind every substep, as it does while a joint has a damper
    // (joints.damping); with neither a world enqueues what it enqueued before.  dp_scratch: the joint part's results, [6][stride]
    struct BodyDamping {
        bool on = false;
        void clear() { *this = BodyDamping{}; }
    } damping;
    DeviceBuffer dp_rows, dp_scratch;
    bool damping_on() const { return damping.on || joints.damping.n != 0; }
    xpbd::DampingTables damping_tables() const
    {
        return xpbd::DampingTables{damping.on ? dp_rows.as<double>() : nullptr, at_least_one(n), joints.damping.n ? joints.damping.table.as<double2>() : nullptr,
                                   dp_scratch.as<double>()};
    }
    // xpbd_world_set_kinematics: the fixed bodies that move on a script.  Non-empty, the step runs the unfused schedule with the
    // velocity overwrite before every integrate stage; empty, a world holds and enqueues nothing of it
    KinematicBodies kinematics;
    // xpbd_world_set_sensors: the bodies that report their pairs and solve none.  None flagged, a world enqueues nothing of it
    Sensors sensors;
    // xpbd_world_set_terrain: the plane table of the heightfield and its description (planes == NULL: none).  World-level, as the
    // contact pad: it names no body, so no upload, population change or restore touches it.  With one the step runs the unfused
    // schedule (the fused pair-solve + integrate + ground kernel has no terrain form).
    xpbd::Terrain terrain{};
    DeviceBuffer tr_planes;
    DeviceBuffer tr_heights; // the heights the table was made from, ny rows of nx: the terrain distance queries read the samples
    TerrainStaging terrain_staging; // of xpbd_world_sample_terrain
    // scene queries (xpbd_world_raycast*, xpbd_world_overlap*): scratch of one call, staging of the host variants' arrays
    xpbd::SceneQueryScratch query;
    // body edits (xpbd_world_set_external_wrench, _apply_impulses, _set_dynamics, _get_dynamics, _set / _get_mass_properties): the
    // staging of the host variants' indices, values (force + torque, or rows of 13 doubles) and impulse lists
    EditStaging edit;
    // body population (xpbd_world_remove_bodies, _add_bodies): the removal flags and index list of the host variant, the scan,
    // old_to_new and its inverse src[new] = old.  Scratch of one call; the new arrays are staged in buffers of their own.
    PopulationScratch pop;
    // state history (xpbd_world_history_*): `length` slots of history_slot_bytes() in one growing block
    History history;
    // contact islands (xpbd_world_islands, _islands_device): scratch of one call; a world that never calls them holds none
    Islands islands;
    // island sleeping (xpbd_world_set_sleeping): off, a world holds and enqueues nothing of it
    Sleep sleep;
    size_t history_slot_bytes() const
    {
        return ((size_t)xpbd::kDynFields * stride * 8 + (size_t)stride * 4 + (sleep.on ? Sleep::state_bytes(stride) : 0) + 255) / 256 * 256;
    }

    // frame_set: which of the two frame sets the substep reads (always 0 outside step_contacts)
    xpbd::ContactBuffers contact_buffers(uint32_t frame_set = 0) const
    {
        xpbd::ContactBuffers c{};
        bp.fill(c);
        c.rec = (frame_set ? cb_rec_b : cb_rec).as<double>();
        c.stat_rec = stat_shared ? cb_stat_shape.as<double>() : cb_stat_rec.as<double>();
        c.stat_index = stat_shared ? shape_id.as<uint32_t>() : nullptr;
        c.stats = np.stats.as<unsigned long long>();
        joints.fill(c);
        c.filter = filters.on ? ft_filters.as<uint2>() : nullptr;
        c.slot_filter = filters.on ? bp.slot_filter.as<uint32_t>() : nullptr;
        c.filter_jointed = (filters.flags & XPBD_FILTER_JOINTED) ? 1u : 0u;
        c.max_depenetration_speed = max_depenetration_speed;
        c.friction = materials.on ? mt_friction.as<double>() : nullptr;
        c.ground_friction = materials.ground_friction;
        c.restitution = restitution.on ? rs_restitution.as<double>() : nullptr;
        c.ground_restitution = restitution.ground;
        c.bounce_threshold = restitution.bounce_threshold;
        c.terrain = terrain;
        return c;
    }

    // What the launches that solve or bounce are handed (both forms of the pair solve, restitution): `c` with the pair codes
    // masked for the sensor pairs (narrowphase_contacts fills the copy behind every narrowphase); no sensor: `c` itself.
    xpbd::ContactBuffers solve_buffers(xpbd::ContactBuffers c) const
    {
        if (sensors.any())
            c.pair_codes = sensors.solve_codes.as<uint8_t>();
        return c;
    }

    // who is inert in the coming frame, for the broadphase (sleeping off: nobody, the kernels of a world without sleeping)
    xpbd::InertBodies inert_bodies() const
    {
        return sleep.on ? xpbd::InertBodies{sleep.view(this).inert, bp.slot_inert.as<uint8_t>()} : xpbd::InertBodies{};
    }

    xpbd::BodyArrays arrays() const
    {
        return xpbd::BodyArrays{dyn.as<double>(), stat.as<double>(), shape_id.as<uint32_t>(), stride, n};
    }

    // Nothing queued may outlive the members: the stream is waited for first.  Then, in this order, the pinned blocks and the
    // event of the owners, the stream, and -- as the members go -- the device buffers.  (An owner's destructor releases its
    // host side again, which is then a no-op.)
    ~xpbd_world()
    {
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        bp.release_host();
        report.release_host();
        if (own_stream)
            (void)hipStreamDestroy(own_stream);
    }
};

#pragma GCC visibility push(hidden)

// The sections of Sleep::state and ::scratch for a world of w->stride (valid once ensure() has run).
inline xpbd::SleepState Sleep::view(const xpbd_world *w) const
{
    const size_t st = w->stride;
    xpbd::SleepState s{};
    s.rest_frames = state.as<uint32_t>();
    s.group = s.rest_frames + st;
    s.mark = s.group + st;
    s.ctrl = s.mark + st;
    s.asleep = reinterpret_cast<uint8_t *>(s.ctrl + xpbd::kSleepCtrlWords);
    s.island_min = scratch.as<uint32_t>();
    s.fixed = reinterpret_cast<uint8_t *>(s.island_min + st);
    s.inert = s.fixed + st;
    s.moving = s.inert + st;
    s.n = w->n;
    s.stride = w->stride;
    return s;
}

inline int bind_device(const xpbd_world *w)
{
    XPBD_HIP_TRY(hipSetDevice(w->device));
    return XPBD_OK;
}

// ---- xpbd_world.cpp ---------------------------------------------------------------------------------------------------------
// Do all bodies of a shape share their mass properties bit for bit?  (see stat_shared)
void absorb_stat_record(xpbd_world *w, const xpbd_rigid &body, uint32_t sid);
void reset_stat_records(xpbd_world *w, bool start_over, uint32_t n);
// What a new set or count of bodies does to the world.
void take_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id);
void drop_body_settings(xpbd_world *w);
int adopt_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id);
// Staged uploads: a block of its own / moved over `table` once nothing can fail; all four joint tables from a JointSet.
int stage_upload(DeviceBuffer &fresh, const void *values, size_t bytes);
int upload_table(DeviceBuffer &table, const void *values, size_t bytes);
int stage_joint_tables(xpbd::JointSet set, uint32_t n_bodies, hipStream_t stream, JointTables &out);

// ---- xpbd_world_joint_state.cpp ---------------------------------------------------------------------------------------------
// Targets set on the device go back into joints.set.drives (no-op unless extras.targets_on_device).  Device bound, stream idle.
int sync_drive_targets(xpbd_world *w);

// ---- xpbd_world_kinematic.cpp -----------------------------------------------------------------------------------------------
// Rows set on the device go back into kinematics.list (no-op unless targets_on_device).  Device bound, stream idle.
int sync_kinematic_targets(xpbd_world *w);

// ---- xpbd_world_sensors.cpp -------------------------------------------------------------------------------------------------
// The contact edges of the current report frame for the islands and the sleep pass: the report's keys, compacted now if they are
// not, or -- with sensors -- those of them without a sensor end; their count stays on the device.  Enqueues only (it waits only
// when the scratch of the second form has to grow).  The frame has pairs (w->bp.n_pairs != 0).
int contact_edge_keys(xpbd_world *w, const unsigned long long **keys, const uint32_t **key_count);
// Behind a substep's narrowphase: the masked pair codes for the launches that solve (no sensor: nothing).
int sensor_mask_codes(xpbd_world *w, const xpbd::ContactBuffers &c);
// Behind launch_sleep_frame_begin: a sensor is not inert (no sensor: nothing).
int sensor_not_inert(xpbd_world *w);

// ---- xpbd_world_contacts.cpp ------------------------------------------------------------------------------------------------
int build_neighbours_enqueue(xpbd_world *w, double dt);
int build_neighbours_collect(xpbd_world *w);
int build_neighbours(xpbd_world *w, double dt);
int narrowphase_contacts(xpbd_world *w, const xpbd::BodyArrays &b, const xpbd::ContactBuffers &c);
// kinematic_left: the substeps of the frame still to run, this one included, when the kinematic overwrite belongs before this
// substep's integrate stage (0: not -- no table, or the frame's first substep, whose overwrite precedes the broadphase)
int substep_contacts(xpbd_world *w, double h, uint32_t *trace, uint32_t trace_row, const xpbd::BodySubset &awake = xpbd::BodySubset(),
                     uint32_t kinematic_left = 0);
int step_contacts(xpbd_world *w, double dt, double h, uint32_t substeps, uint32_t *trace);

#pragma GCC visibility pop
