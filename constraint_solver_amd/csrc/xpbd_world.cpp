// xpbd_world.cpp -- implementation of the C ABI in include/xpbd.h.
//
// Owns the device-side SoA body arrays, the shape tables and the HIP stream of
// one world, and turns each ABI call into kernel launches from xpbd_kernels.hip.
// There is no CPU fallback: without a usable HIP device every compute entry
// point fails with XPBD_E_NO_DEVICE / XPBD_E_HIP.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "xpbd_internal.h"
#include "xpbd_kernels.h"
#include "xpbd_math.hpp"
#include "xpbd_contacts.h"
#include "xpbd_gjk.h"
#include "xpbd_pairs.h"
#include "xpbd_population.h"
#include "xpbd_population_remap.hpp"
#include "xpbd_query.h"
#include "xpbd_report.h"

namespace {

uint32_t round_up(uint32_t v, uint32_t to) { return (v + to - 1) / to * to; }

} // namespace

using xpbd::DeviceBuffer;
using xpbd::set_error;

// The joints of a world: what the caller handed to xpbd_world_set_joints, _set_joint_limits and _set_joint_drives, and the
// device tables built from it in three parts, one per setter.  A part is complete or empty (count 0, no buffers); only
// stage_csr, stage_limits and stage_extras fill one, aside, and a setter or a population change moves it in.
namespace {
struct JointTables {
    xpbd::JointSet set;                         // joints, limits of all kinds and drives, the caller's order (limits and drives name
                                                // joints by index: new joints drop them; a population change re-indexes all three)
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
    } extras;

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
    void clear() { *this = JointTables{}; }
};
} // namespace

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
    uint32_t max_shape_id = 0; // largest shape id among the uploaded bodies (xpbd_world_set_shapes re-validates against it)
    DeviceBuffer dyn, stat, shape_id, aos_staging, last_mask, trace, block_counts, contacts;
    uint32_t trace_rows = 0; // substeps recorded by the last step()
    bool stepped = false;

    // shapes
    DeviceBuffer shape_verts, shape_offsets;
    uint32_t n_shapes = 0, total_verts = 0;

    // extension: polytope topology for the body-body narrowphase
    DeviceBuffer planes, centroids, shape_desc, face_start, face_verts, edges, pair_buf, manifold_buf;
    DeviceBuffer shape_radii, edge_dirs, edge_dir_id, shape_class;
    uint32_t two_classes = 0, small_max_face_verts = 0;
    bool has_topology = false;
    uint32_t max_verts = 0, max_faces = 0, max_face_verts = 0;
    xpbd::PolytopeTables tables() const
    {
        return xpbd::PolytopeTables{shape_verts.as<double>(), planes.as<double>(), centroids.as<double>(),
                                    shape_desc.as<xpbd::ShapeDesc>(), face_start.as<uint32_t>(),
                                    face_verts.as<uint32_t>(), edges.as<uint32_t>(), shape_radii.as<double>(),
                                    edge_dirs.as<double>(), edge_dir_id.as<uint32_t>(), n_shapes, total_verts, max_verts, max_faces, max_face_verts,
                                    shape_class.as<uint8_t>(), two_classes, small_max_face_verts};
    }

    // extension: contact pipeline (XPBD_MODE_CONTACTS)
    double contact_pad = 0.02;
    double max_depenetration_speed = 0.0; // 0 = off (the reference's solver loop)
    uint32_t narrowphase = XPBD_NARROWPHASE_SAT;
    DeviceBuffer dyn_alt, cb_centers, cb_radius, cb_cell, cb_key, cb_maxr, cb_bucket_start, cb_bucket_cursor, cb_items,
        cb_nbr_off, cb_pair_first, cb_upper_start, cb_nbr, cb_nbr_pair, cb_pairs, cb_rec, cb_stat_rec,
        cb_manifolds, cb_stats, cb_scan, cb_slot_sphere, cb_slot_cell;
    // second set of per-substep records for the fused "end of substep k + start of substep k + 1" kernel (step_contacts)
    DeviceBuffer cb_rec_b;
    bool stat_rec_valid = false; // the StatRecords mirror the SoA static fields of the bodies uploaded last
    // Mass properties shared per shape: when every body of a shape has bit-identical inverse mass, inverse inertia and
    // centre of mass (checked on the host at upload -- the usual case: bodies are instances of a few shapes), the contact
    // kernels read them from a table of n_shapes StatRecords indexed by shape id (cache resident) instead of gathering a
    // 128-byte record per body and per neighbour.  Same values, so the same bits.
    bool stat_shared = false;
    std::vector<double> stat_shape_host; // [n_shapes][kStatRecDoubles]
    std::vector<uint8_t> stat_shape_seen; // [n_shapes] a body of the shape has been uploaded: its row of stat_shape_host is set
    // re-packing the bodies on the device (xpbd::repack_bodies): the new world in AoS, its shape ids, the source map, incoming records
    DeviceBuffer repack_aos, repack_shape, repack_src, repack_incoming, halo_keys, halo_records;
    DeviceBuffer cb_stat_shape;
    DeviceBuffer cb_grid_partials, cb_items_unsorted;
    uint32_t table_size = 0, n_entries = 0, n_pairs = 0;
    bool have_neighbours = false;
    // The broadphase in two halves (build_neighbours_enqueue / _collect): the counting kernels leave the totals the host
    // needs to size the pair buffers in PINNED memory and record an event; only the second half waits for it.  A host that
    // drives several worlds (xpbd_multi.cpp: one per GPU) enqueues all of them before it waits for any.
    struct BroadphaseTotals {
        uint32_t entries, pairs;
        unsigned long long stats[2];
    };
    BroadphaseTotals *bp_totals = nullptr; // hipHostMalloc
    hipEvent_t bp_event = nullptr;
    bool bp_pending = false;
    // state at the start of a frame (xpbd::frame_snapshot_save / _restore): the 13 dynamic fields and the contact masks
    DeviceBuffer frame_snapshot;
    bool frame_snapshot_valid = false, frame_snapshot_stepped = false;
    // Body-indexed settings: each names bodies (or the joints between them) by index, so a new set of bodies clears all four
    // (adopt_body_count).  Values whose clear() restores the defaults; the per-body device tables stay allocated beside theirs.
    JointTables joints;
    struct Filters { // xpbd_world_set_collision_filters: group, mask per body (on), XPBD_FILTER_* flags
        bool on = false;
        uint32_t flags = 0;
        void clear() { *this = Filters{}; }
    } filters;
    DeviceBuffer ft_filters, cb_slot_filter;
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
    // xpbd_world_set_terrain: the plane table of the heightfield and its description (planes == NULL: none).  World-level, as the
    // contact pad: it names no body, so no upload, population change or restore touches it.  With one the step runs the unfused
    // schedule (the fused pair-solve + integrate + ground kernel has no terrain form).  tr_xy, tr_out: staging of xpbd_world_sample_terrain.
    xpbd::Terrain terrain{};
    DeviceBuffer tr_planes, tr_xy, tr_out;
    // scene queries (xpbd_world_raycast*, xpbd_world_overlap*): scratch of one call, staging of the host variants' arrays
    xpbd::SceneQueryScratch query;
    // body edits (xpbd_world_set_external_wrench, _apply_impulses, _set_dynamics, _get_dynamics): the staging of the host
    // variants' indices, values (force + torque, or rows of 13 doubles) and impulse lists
    DeviceBuffer ed_indices, ed_values, ed_list;
    // body population (xpbd_world_remove_bodies, _add_bodies): the removal flags and index list of the host variant, the scan,
    // old_to_new and its inverse src[new] = old.  Scratch of one call; the new arrays are staged in buffers of their own.
    DeviceBuffer pop_remove, pop_indices, pop_prefix, pop_scan, pop_map, pop_src;
    // state history (xpbd_world_history_*): `history_length` slots of history_slot_bytes() in one growing block
    DeviceBuffer history;
    uint32_t history_length = 0;
    std::vector<uint8_t> history_stepped;
    size_t history_slot_bytes() const { return ((size_t)xpbd::kDynFields * stride * 8 + (size_t)stride * 4 + 255) / 256 * 256; }
    // SAT in two passes (pre-test pass + survivor list, xpbd_pairs.h): chosen per frame from the share of touching
    // pairs in the previous frame, read back at the broadphase's synchronisation point
    DeviceBuffer sat_counters, sat_survivors, sat_axis_cache, gjk_axis_cache, cb_pair_codes;
    xpbd::SatScratch sat_scratch{nullptr, nullptr, 0, nullptr, true};
    bool sat_two_pass = false;
    uint32_t sat_schedule = XPBD_SAT_SCHEDULE_AUTO;
    unsigned long long stats_touching_seen = 0, stats_pair_substeps = 0, stats_pair_substeps_seen = 0;
    DeviceBuffer gjk_counters, gjk_pairs_scratch;   // hit list of the two-kernel GJK/EPA narrowphase (xpbd_gjk.h)
    xpbd::GjkScratch gjk_scratch{nullptr, nullptr, 0, nullptr, nullptr};
    // contact reports (xpbd_world_set_contact_report; xpbd_report.h).  rep_keys[report_cur] holds this frame's touching
    // pairs once compacted, rep_keys[report_cur ^ 1] those of the previous frame (S_prev, when report_prev_valid).
    bool report_on = false;
    bool report_frame = false;      // the current pair list counts its touching substeps in rep_touch (zeroed by its broadphase)
    bool report_keys_ready = false; // rep_keys[report_cur] is up to date with the substeps run (its count on its way to rep_host)
    bool report_ready = false;      // report_counts and the scans behind them are up to date
    bool report_prev_valid = false;
    uint32_t report_substeps = 0, report_cur = 0;
    uint32_t report_counts[4] = {0, 0, 0, 0}; // pairs, points, begins, ends
    uint32_t *rep_host = nullptr;   // hipHostMalloc: [0..1] key counts of rep_keys[0..1], [2..4] point / BEGIN / event totals
    DeviceBuffer rep_touch, rep_flag, rep_sel, rep_npts, rep_keys[2], rep_scan, rep_ev_flag, rep_pairs, rep_points, rep_events;
    // a shard of the multi-GPU world, for the duration of xpbd::report_shard only: owned slots and global ids (ReportFrame)
    const uint8_t *rep_map_owned = nullptr;
    const uint32_t *rep_map_ids = nullptr;
    // frame_set: which of the two frame sets the substep reads (always 0 outside step_contacts)
    xpbd::ContactBuffers contact_buffers(uint32_t frame_set = 0) const
    {
        xpbd::ContactBuffers c{};
        c.centers = cb_centers.as<double>();
        c.radius = cb_radius.as<double>();
        c.cell = cb_cell.as<int32_t>();
        c.key = cb_key.as<uint32_t>();
        c.grid = cb_maxr.as<xpbd::GridInfo>();
        c.grid_partials = cb_grid_partials.as<double>();
        c.bucket_start = cb_bucket_start.as<uint32_t>();
        c.bucket_cursor = cb_bucket_cursor.as<uint32_t>();
        c.items = cb_items.as<uint32_t>();
        c.items_unsorted = cb_items_unsorted.as<uint32_t>();
        c.table_size = table_size;
        c.slot_sphere = cb_slot_sphere.as<double>();
        c.slot_cell = cb_slot_cell.as<int32_t>();
        c.nbr_off = cb_nbr_off.as<uint32_t>();
        c.pair_first = cb_pair_first.as<uint32_t>();
        c.upper_start = cb_upper_start.as<uint32_t>();
        c.nbr = cb_nbr.as<uint32_t>();
        c.nbr_pair = cb_nbr_pair.as<uint32_t>();
        c.pairs = cb_pairs.as<uint32_t>();
        c.rec = (frame_set ? cb_rec_b : cb_rec).as<double>();
        c.stat_rec = stat_shared ? cb_stat_shape.as<double>() : cb_stat_rec.as<double>();
        c.stat_index = stat_shared ? shape_id.as<uint32_t>() : nullptr;
        c.manifolds = cb_manifolds.as<xpbd::ContactManifold>();
        c.pair_codes = cb_pair_codes.as<uint8_t>();
        c.stats = cb_stats.as<unsigned long long>();
        c.scan_scratch = cb_scan.as<uint32_t>();
        joints.fill(c);
        c.filter = filters.on ? ft_filters.as<uint2>() : nullptr;
        c.slot_filter = filters.on ? cb_slot_filter.as<uint32_t>() : nullptr;
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

    xpbd::BodyArrays arrays() const
    {
        return xpbd::BodyArrays{dyn.as<double>(), stat.as<double>(), shape_id.as<uint32_t>(), stride, n};
    }
    xpbd::ShapeTable shapes() const
    {
        return xpbd::ShapeTable{shape_verts.as<double>(), shape_offsets.as<uint32_t>(), n_shapes, total_verts};
    }

    ~xpbd_world() // (then the device buffers free themselves)
    {
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        if (bp_totals)
            (void)hipHostFree(bp_totals);
        if (bp_event)
            (void)hipEventDestroy(bp_event);
        if (rep_host)
            (void)hipHostFree(rep_host);
        if (own_stream)
            (void)hipStreamDestroy(own_stream);
    }
};

namespace {

constexpr uint32_t kDefaultBlock = 64;

int bind_device(const xpbd_world *w)
{
    XPBD_HIP_TRY(hipSetDevice(w->device));
    return XPBD_OK;
}

uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v)
        p <<= 1;
    return p;
}

// Scratch of launch_gjk_epa_pairs for `n_pairs` pairs (growing it frees the old block, which waits for the device).
int ensure_gjk_scratch(xpbd_world *w, uint32_t n_pairs)
{
    if (!w->gjk_counters.ptr) {
        XPBD_HIP_TRY(w->gjk_counters.reserve(xpbd::gjk_counter_bytes()));
        XPBD_HIP_TRY(hipMemsetAsync(w->gjk_counters.ptr, 0, xpbd::gjk_counter_bytes(), w->stream));
        w->gjk_scratch.calls = 0;
    }
    XPBD_HIP_TRY(w->gjk_pairs_scratch.reserve(xpbd::gjk_scratch_bytes(n_pairs ? n_pairs : 1)));
    w->gjk_scratch.counters = w->gjk_counters.as<uint32_t>();
    w->gjk_scratch.pairs_scratch = w->gjk_pairs_scratch.ptr;
    return XPBD_OK;
}

// ---- contact reports (xpbd_world_set_contact_report; semantics in include/xpbd.h) ---------------------------------------------
// Nothing starts a frame, no touch count, no scan runs while reporting is off.
void report_reset(xpbd_world *w)
{
    w->report_frame = w->report_keys_ready = w->report_ready = w->report_prev_valid = false;
    w->report_substeps = 0;
}

xpbd::ReportFrame report_frame_of(const xpbd_world *w)
{
    return xpbd::ReportFrame{w->cb_pairs.as<uint32_t>(), w->cb_pair_codes.as<uint8_t>(), w->cb_manifolds.as<xpbd::ContactManifold>(),
                             w->rep_touch.as<uint32_t>(), w->n_pairs, w->rep_map_owned, w->rep_map_ids};
}

// This frame's touching pairs -> rep_keys[report_cur]; their count travels to rep_host[report_cur].  Enqueued only.
int report_compact_keys(xpbd_world *w)
{
    const uint32_t cur = w->report_cur;
    XPBD_HIP_TRY(xpbd::launch_report_keys(report_frame_of(w), w->rep_flag.as<uint32_t>(), w->rep_scan.as<uint32_t>(),
                                          w->rep_keys[cur].as<unsigned long long>(), w->rep_sel.as<uint32_t>(), w->rep_npts.as<uint32_t>(),
                                          w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->rep_host[cur], w->rep_flag.as<uint32_t>() + w->n_pairs, 4, hipMemcpyDeviceToHost, w->stream));
    w->report_keys_ready = true;
    return XPBD_OK;
}

// Before a broadphase replaces the pair list: the frame's touching set becomes the next frame's S_prev (a frame without a
// substep touched nothing).  The keys must be compacted now -- the pairs, codes and counters they come from are rebuilt.
int report_frame_end(xpbd_world *w)
{
    if (!w->report_on)
        return XPBD_OK;
    if (w->report_frame && w->report_substeps) {
        if (!w->report_keys_ready)
            XPBD_TRY(report_compact_keys(w));
        w->report_prev_valid = true;
        w->report_cur ^= 1u;
    } else {
        w->report_prev_valid = false; // a frame without a substep touched nothing; and after an enable, upload, restore or failure S_prev is empty
    }
    w->report_frame = w->report_keys_ready = w->report_ready = false;
    w->report_substeps = 0;
    return XPBD_OK;
}

// After the broadphase has sized the pair list: the counters of the new frame start at zero.
int report_frame_begin(xpbd_world *w)
{
    if (!w->report_on)
        return XPBD_OK;
    const size_t np = w->n_pairs ? w->n_pairs : 1;
    XPBD_HIP_TRY(w->rep_touch.reserve(np * 4));
    XPBD_HIP_TRY(w->rep_flag.reserve((np + 1) * 4));
    XPBD_HIP_TRY(w->rep_sel.reserve(np * 4));
    XPBD_HIP_TRY(w->rep_npts.reserve((np + 1) * 4));
    XPBD_HIP_TRY(w->rep_keys[w->report_cur].reserve(np * 8)); // (the other one holds S_prev)
    XPBD_HIP_TRY(w->rep_scan.reserve((np / 1024 + 8) * 4));
    XPBD_HIP_TRY(hipMemsetAsync(w->rep_touch.ptr, 0, np * 4, w->stream));
    w->report_frame = true;
    w->report_keys_ready = w->report_ready = false;
    w->report_substeps = 0;
    return XPBD_OK;
}

// Everything a count or download needs of the current frame: keys, point offsets, event flags and their totals.  Waits.
int report_prepare(xpbd_world *w, const char *who)
{
    if (!w->report_on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_world_set_contact_report)", who);
    if (!w->report_frame || !w->report_substeps)
        return set_error(XPBD_E_INVALID, "%s: no report: no substep of XPBD_MODE_CONTACTS has run since the last broadphase, upload, "
                                         "history restore, enable, failed step or step in another mode", who);
    if (w->report_ready)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    if (!w->report_keys_ready)
        XPBD_TRY(report_compact_keys(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // (also: reserve() frees a block only when no queued work uses it)
    const uint32_t cur = w->report_cur, k = w->rep_host[cur], n_prev = w->report_prev_valid ? w->rep_host[cur ^ 1u] : 0u;
    const size_t n_ev = (size_t)k + n_prev;
    XPBD_HIP_TRY(w->rep_ev_flag.reserve((n_ev + 1) * 4));
    XPBD_HIP_TRY(w->rep_scan.reserve((n_ev / 1024 + 8) * 4)); // both scans below: k <= n_ev
    XPBD_HIP_TRY(xpbd::launch_exclusive_scan(w->rep_npts.as<uint32_t>(), k, w->rep_scan.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_report_event_flags(w->rep_keys[cur].as<unsigned long long>(), k, w->rep_keys[cur ^ 1u].as<unsigned long long>(),
                                                 n_prev, w->rep_ev_flag.as<uint32_t>(), w->rep_scan.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->rep_host[2], w->rep_npts.as<uint32_t>() + k, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->rep_host[3], w->rep_ev_flag.as<uint32_t>() + k, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->rep_host[4], w->rep_ev_flag.as<uint32_t>() + n_ev, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    w->report_counts[0] = k;
    w->report_counts[1] = w->rep_host[2];
    w->report_counts[2] = w->rep_host[3];
    w->report_counts[3] = w->rep_host[4] - w->rep_host[3];
    w->report_ready = true;
    return XPBD_OK;
}

// Sphere broadphase of the contact pipeline: neighbour lists + pair list for the coming frame, in two halves.
// First half: bounding spheres, buckets and the neighbour COUNT of every body are enqueued, the totals travel to pinned host
// memory behind them, an event marks their arrival.  Nothing here waits for the device.
int build_neighbours_enqueue(xpbd_world *w, double dt)
{
    if (int rc = report_frame_end(w))
        return rc;
    if (!w->bp_totals) {
        XPBD_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->bp_totals), sizeof *w->bp_totals, hipHostMallocDefault));
        XPBD_HIP_TRY(hipEventCreateWithFlags(&w->bp_event, hipEventDisableTiming));
    }
    const uint32_t n = w->n, st = w->stride;
    w->table_size = next_pow2(n < 512 ? 1024 : 2 * n);
    XPBD_HIP_TRY(w->cb_centers.reserve((size_t)3 * st * 8));
    XPBD_HIP_TRY(w->cb_radius.reserve((size_t)st * 8));
    XPBD_HIP_TRY(w->cb_cell.reserve((size_t)3 * st * 4));
    XPBD_HIP_TRY(w->cb_key.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->cb_maxr.reserve(sizeof(xpbd::GridInfo)));
    XPBD_HIP_TRY(w->cb_grid_partials.reserve(((size_t)st / 256 + 1) * 7 * 8));
    XPBD_HIP_TRY(w->cb_bucket_start.reserve((size_t)(w->table_size + 1) * 4));
    XPBD_HIP_TRY(w->cb_bucket_cursor.reserve((size_t)w->table_size * 4));
    XPBD_HIP_TRY(w->cb_items.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->cb_items_unsorted.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->cb_slot_sphere.reserve((size_t)4 * st * 8));
    XPBD_HIP_TRY(w->cb_slot_cell.reserve((size_t)3 * st * 4));
    if (w->filters.on)
        XPBD_HIP_TRY(w->cb_slot_filter.reserve((size_t)2 * st * 4));
    XPBD_HIP_TRY(w->cb_nbr_off.reserve((size_t)(st + 1) * 4));
    XPBD_HIP_TRY(w->cb_pair_first.reserve((size_t)(st + 1) * 4));
    XPBD_HIP_TRY(w->cb_upper_start.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * st * 8));
    XPBD_HIP_TRY(w->cb_rec_b.reserve((size_t)xpbd::kRecDoubles * st * 8));
    if (w->stat_shared) {
        if (!w->stat_rec_valid) {
            XPBD_HIP_TRY(w->cb_stat_shape.reserve(w->stat_shape_host.size() * 8));
            XPBD_HIP_TRY(hipMemcpyAsync(w->cb_stat_shape.ptr, w->stat_shape_host.data(), w->stat_shape_host.size() * 8,
                                        hipMemcpyHostToDevice, w->stream));
            XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // (pageable source)
            w->stat_rec_valid = true;
        }
    } else {
        if (w->cb_stat_rec.bytes < (size_t)xpbd::kStatRecDoubles * st * 8)
            w->stat_rec_valid = false;
        XPBD_HIP_TRY(w->cb_stat_rec.reserve((size_t)xpbd::kStatRecDoubles * st * 8));
        if (!w->stat_rec_valid) {
            XPBD_HIP_TRY(xpbd::launch_stat_records(w->arrays(), w->cb_stat_rec.as<double>(), w->stream));
            w->stat_rec_valid = true;
        }
    }
    XPBD_HIP_TRY(w->cb_scan.reserve(((size_t)(w->table_size > st ? w->table_size : st) / 1024 + 8) * 4));
    if (!w->cb_stats.ptr) {
        XPBD_HIP_TRY(w->cb_stats.reserve(16));
        XPBD_HIP_TRY(hipMemsetAsync(w->cb_stats.ptr, 0, 16, w->stream));
        w->stats_touching_seen = 0;
        w->stats_pair_substeps_seen = w->stats_pair_substeps;
    }
    const xpbd::BodyArrays b = w->arrays();
    xpbd::ContactBuffers c = w->contact_buffers();
    XPBD_HIP_TRY(xpbd::launch_bounds_and_cells(b, w->tables(), w->shape_radii.as<double>(), dt, w->contact_pad, c,
                                               w->stream));
    XPBD_HIP_TRY(xpbd::launch_build_buckets(b, c, w->stream));
    XPBD_HIP_TRY(xpbd::launch_neighbour_count(b, c, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->bp_totals->entries, c.nbr_off + n, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->bp_totals->pairs, c.pair_first + n, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->bp_totals->stats, c.stats, 16, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipEventRecord(w->bp_event, w->stream));
    w->bp_pending = true;
    w->have_neighbours = false;
    return XPBD_OK;
}

// Second half: waits for the totals (the one host synchronisation of a frame in XPBD_MODE_CONTACTS), sizes the pair
// buffers and fills the neighbour and pair lists.
int build_neighbours_collect(xpbd_world *w)
{
    if (!w->bp_pending)
        return set_error(XPBD_E_INVALID, "build_neighbours_collect without build_neighbours_enqueue");
    XPBD_HIP_TRY(hipEventSynchronize(w->bp_event));
    w->bp_pending = false;
    const xpbd::BodyArrays b = w->arrays();
    xpbd::ContactBuffers c = w->contact_buffers();
    const unsigned long long stats_now[2] = {w->bp_totals->stats[0], w->bp_totals->stats[1]};
    w->n_entries = w->bp_totals->entries;
    w->n_pairs = w->bp_totals->pairs;
    {
        // Pre-test as a pass of its own for the coming frame?  Either way the results are the same bits; this only
        // picks the cheaper schedule from how many of the pairs examined since the last broadphase were touching.
        // SAT: the pre-test pass also answers the pairs whose cached face axis still separates them (SatScratch), so it
        // pays unless nearly every pair touches (box stacks: 99 % touching, one pass 5 % faster; a pile of boxes with
        // 40 % touching: two passes 35 % faster).  (GJK + EPA always runs the pre-test as a pass of its own: see
        // narrowphase_contacts.)
        const unsigned long long touching = stats_now[0] - w->stats_touching_seen;
        const unsigned long long examined = w->stats_pair_substeps - w->stats_pair_substeps_seen;
        if (w->sat_schedule != XPBD_SAT_SCHEDULE_AUTO)
            w->sat_two_pass = w->sat_schedule == XPBD_SAT_SCHEDULE_TWO_PASS;
        else if (examined)
            w->sat_two_pass = touching * 5 < examined * 4;
        if (w->sat_schedule == XPBD_SAT_SCHEDULE_AUTO && w->two_classes)
            w->sat_two_pass = true; // small and large shapes: the two-pass form sorts the pairs by class (xpbd_pairs.h)
        // A DENSE scene (>= 15 % of the pairs examined in the last frame touched)?  Then (a) separating EDGE axes go into the
        // axis cache (SatScratch): trying one costs the pre-test a whole edge query for every wave that holds such a pair; it
        // pays where many pairs are close (piles: 35-40 % of the pairs touch, +4 % / +9 %), not where a few are (chains of
        // spaced boxes: 5 % touch, -4 %); and (b) box pairs run in groups of four lanes instead of eight (for_shape_maxima:
        // piles and stacks +7 %, the chains -3 %).  Same bits either way.
        if (examined)
            w->sat_scratch.cache_edge_axes = touching * 100 >= examined * 15;
        w->stats_touching_seen = stats_now[0];
        w->stats_pair_substeps_seen = w->stats_pair_substeps;
    }
    if (!w->sat_counters.ptr) {
        XPBD_HIP_TRY(w->sat_counters.reserve(2 * xpbd::kSurvivorCounters * 4));
        XPBD_HIP_TRY(hipMemsetAsync(w->sat_counters.ptr, 0, 2 * xpbd::kSurvivorCounters * 4, w->stream));
        w->sat_scratch.calls = 0;
    }
    XPBD_HIP_TRY(w->sat_survivors.reserve((size_t)(w->n_pairs ? w->n_pairs : 1) * 2 * 4)); // 2 * n_pairs entries: SatScratch
    // the pair list is new: nothing is known about which axis separates which pair
    XPBD_HIP_TRY(w->sat_axis_cache.reserve((size_t)(w->n_pairs ? w->n_pairs : 1) * 2));
    XPBD_HIP_TRY(hipMemsetAsync(w->sat_axis_cache.ptr, 0, (size_t)(w->n_pairs ? w->n_pairs : 1) * 2, w->stream));
    w->sat_scratch.counters = w->sat_counters.as<uint32_t>();
    w->sat_scratch.survivors = w->sat_survivors.as<uint32_t>();
    w->sat_scratch.axis_cache = w->sat_axis_cache.as<uint16_t>();
    if (w->narrowphase == XPBD_NARROWPHASE_GJK_EPA) {
        XPBD_HIP_TRY(w->gjk_axis_cache.reserve((size_t)(w->n_pairs ? w->n_pairs : 1) * 24));
        XPBD_HIP_TRY(hipMemsetAsync(w->gjk_axis_cache.ptr, 0, (size_t)(w->n_pairs ? w->n_pairs : 1) * 24, w->stream));
    }
    XPBD_HIP_TRY(w->cb_nbr.reserve((size_t)(w->n_entries ? w->n_entries : 1) * 4));
    XPBD_HIP_TRY(w->cb_nbr_pair.reserve((size_t)(w->n_entries ? w->n_entries : 1) * 4));
    XPBD_HIP_TRY(w->cb_pairs.reserve((size_t)(w->n_pairs ? w->n_pairs : 1) * 8));
    XPBD_HIP_TRY(w->cb_manifolds.reserve((size_t)(w->n_pairs ? w->n_pairs : 1) * sizeof(xpbd::ContactManifold)));
    XPBD_HIP_TRY(w->cb_pair_codes.reserve((size_t)(w->n_pairs ? w->n_pairs : 1)));
    c = w->contact_buffers();
    XPBD_HIP_TRY(xpbd::launch_neighbour_fill(b, c, w->stream));
    w->have_neighbours = true;
    return report_frame_begin(w);
}

int build_neighbours(xpbd_world *w, double dt)
{
    if (int rc = build_neighbours_enqueue(w, dt))
        return rc;
    return build_neighbours_collect(w);
}

// Narrowphase of the current substep on the post-integrate frames of `c`.
int narrowphase_contacts(xpbd_world *w, const xpbd::BodyArrays &b, const xpbd::ContactBuffers &c)
{
    if (w->narrowphase == XPBD_NARROWPHASE_GJK_EPA) {
        if (int rc = ensure_gjk_scratch(w, w->n_pairs))
            return rc;
        // always with the pre-test as a pass of its own: that pass consults the cached separating directions, which are
        // part of the narrowphase's semantics (og_gjk_epa_cached of the oracle), not a schedule
        w->gjk_scratch.axis_cache = w->gjk_axis_cache.as<double>();
        w->gjk_scratch.codes = c.pair_codes;
        XPBD_HIP_TRY(xpbd::launch_gjk_epa_pairs(b, w->tables(), c.rec, c.pairs, w->n_pairs, nullptr, c.manifolds,
                                                w->gjk_scratch, true, &w->sat_scratch, w->stream));
    } else {
        XPBD_HIP_TRY(xpbd::launch_sat_contact_pairs(b, w->tables(), c, w->n_pairs, w->sat_two_pass ? &w->sat_scratch : nullptr,
                                                    w->stream, w->sat_scratch.cache_edge_axes /* = a dense scene, see below */));
    }
    w->stats_pair_substeps += w->n_pairs;
    if (w->report_frame) {
        XPBD_HIP_TRY(xpbd::launch_report_touch(c.pair_codes, w->rep_touch.as<uint32_t>(), w->n_pairs, w->stream));
        ++w->report_substeps;
        w->report_keys_ready = w->report_ready = false;
    }
    return XPBD_OK;
}

// One substep of the contact pipeline (neighbour lists must be current): the form the split API
// (xpbd_world_contacts_substep) exposes, with a seam for the halo exchange after it.
int substep_contacts(xpbd_world *w, double h, uint32_t *trace, uint32_t trace_row)
{
    const xpbd::BodyArrays b = w->arrays();
    const xpbd::ContactBuffers c = w->contact_buffers();
    if (c.restitution) {
        // The velocity pass reads, of every body, the velocities the substep started from and the state after derive while it
        // writes its own body's result: the former are copied aside first (fields D_VEL.. of the SoA state are one block), the
        // latter goes to dyn_alt, and the pass writes the SoA state, which nobody reads by then.
        XPBD_HIP_TRY(hipMemcpyAsync(w->rs_start.ptr, b.dyn + (size_t)xpbd::D_VEL * b.stride, (size_t)6 * b.stride * 8, hipMemcpyDeviceToDevice,
                                    w->stream));
    }
    XPBD_HIP_TRY(xpbd::launch_integrate_ground(b, w->shapes(), h, c, w->last_mask.as<uint32_t>(), trace, trace_row, w->stream));
    if (int rc = narrowphase_contacts(w, b, c))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_joint_extras(h, c, w->stream));
    if (!c.restitution) {
        XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, b.dyn, h, c, w->stream));
        return XPBD_OK;
    }
    XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, w->dyn_alt.as<double>(), h, c, w->stream));
    XPBD_HIP_TRY(xpbd::launch_restitution(b, w->dyn_alt.as<double>(), w->rs_start.as<double>(), w->shapes(), c, w->last_mask.as<uint32_t>(),
                                          w->stream));
    return XPBD_OK;
}

// One xpbd_world_step in XPBD_MODE_CONTACTS (semantics: oracle/xpbd_pairs_oracle.h).  All substeps run here, so the
// pair solve of substep k and the integrate + ground stage of substep k + 1 are one kernel; the body records alternate
// between two sets because the bodies still read each other's records of substep k while those of k + 1 are written.
// Between the substeps the state lives in the records only; the SoA arrays are read by the first kernel and written by
// the last.
int step_contacts(xpbd_world *w, double dt, double h, uint32_t substeps, uint32_t *trace)
{
    if (!w->has_topology)
        return set_error(XPBD_E_INVALID, "XPBD_MODE_CONTACTS needs xpbd_world_set_polytopes");
    if (int rc = build_neighbours(w, dt))
        return rc;
    if (substeps == 0)
        return XPBD_OK;
    // the velocity pass sits where the fused kernel below has the next substep's integrate; and that kernel has no terrain form
    if (w->restitution.on || w->terrain.planes) {
        for (uint32_t k = 0; k < substeps; ++k)
            if (int rc = substep_contacts(w, h, trace, k))
                return rc;
        return XPBD_OK;
    }
    XPBD_HIP_TRY(xpbd::launch_integrate_ground(w->arrays(), w->shapes(), h, w->contact_buffers(0), w->last_mask.as<uint32_t>(), trace, 0,
                                               w->stream));
    for (uint32_t k = 0; k < substeps; ++k) {
        const xpbd::BodyArrays b = w->arrays();
        const xpbd::ContactBuffers c = w->contact_buffers(k & 1u);
        if (int rc = narrowphase_contacts(w, b, c))
            return rc;
        XPBD_HIP_TRY(xpbd::launch_joint_extras(h, c, w->stream));
        if (k + 1 < substeps) {
            const xpbd::ContactBuffers next = w->contact_buffers((k + 1u) & 1u);
            XPBD_HIP_TRY(xpbd::launch_pair_solve_integrate_ground(b, w->shapes(), h, c, next.rec, w->last_mask.as<uint32_t>(), trace,
                                                                  k + 1, w->stream));
        } else {
            XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, b.dyn, h, c, w->stream));
        }
    }
    return XPBD_OK;
}

} // namespace

// ---- the frame of a multi-GPU shard, split at the halo exchange (xpbd_internal.h) -------------------------------------------
namespace xpbd {

int halo_frame_begin_enqueue(xpbd_world *w, double dt) noexcept
{
    if (!w || w->mode != XPBD_MODE_CONTACTS || !w->has_topology)
        return set_error(XPBD_E_INVALID, "halo_frame_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    return build_neighbours_enqueue(w, dt);
}

int halo_frame_begin_collect(xpbd_world *w, double h) noexcept
{
    if (!w || w->mode != XPBD_MODE_CONTACTS || !w->has_topology)
        return set_error(XPBD_E_INVALID, "halo_frame_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    if (int rc = build_neighbours_collect(w))
        return rc;
    XPBD_HIP_TRY(launch_integrate_ground(w->arrays(), w->shapes(), h, w->contact_buffers(0), w->last_mask.as<uint32_t>(), nullptr, 0, w->stream));
    w->stepped = true;
    return XPBD_OK;
}

// The state a frame starts from -- the 13 dynamic fields of every body and the contact masks of the last substep -- kept
// aside (device to device, on the world's stream) so that a frame whose halos turn out to have been too thin can be undone.
int frame_snapshot_save(xpbd_world *w) noexcept
{
    if (!w)
        return set_error(XPBD_E_INVALID, "frame_snapshot_save: NULL world");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const size_t dyn_bytes = (size_t)kDynFields * w->stride * 8, mask_bytes = (size_t)w->stride * 4;
    if (w->frame_snapshot.bytes < dyn_bytes + mask_bytes) {
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() frees the old block
        XPBD_HIP_TRY(w->frame_snapshot.reserve(dyn_bytes + mask_bytes));
    }
    char *dst = static_cast<char *>(w->frame_snapshot.ptr);
    XPBD_HIP_TRY(hipMemcpyAsync(dst, w->dyn.ptr, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(dst + dyn_bytes, w->last_mask.ptr, mask_bytes, hipMemcpyDeviceToDevice, w->stream));
    w->frame_snapshot_valid = true;
    w->frame_snapshot_stepped = w->stepped;
    return XPBD_OK;
}

int frame_snapshot_restore(xpbd_world *w) noexcept
{
    if (!w)
        return set_error(XPBD_E_INVALID, "frame_snapshot_restore: NULL world");
    if (w->n == 0)
        return XPBD_OK;
    if (!w->frame_snapshot_valid)
        return set_error(XPBD_E_INVALID, "frame_snapshot_restore: no snapshot");
    if (int rc = bind_device(w))
        return rc;
    const size_t dyn_bytes = (size_t)kDynFields * w->stride * 8, mask_bytes = (size_t)w->stride * 4;
    const char *src = static_cast<const char *>(w->frame_snapshot.ptr);
    XPBD_HIP_TRY(hipMemcpyAsync(w->dyn.ptr, src, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->last_mask.ptr, src + dyn_bytes, mask_bytes, hipMemcpyDeviceToDevice, w->stream));
    w->stepped = w->frame_snapshot_stepped;
    w->have_neighbours = false;
    w->bp_pending = false;
    w->trace_rows = 0;
    return XPBD_OK;
}

namespace {
// pair solve (+ next substep's integrate + ground unless `last`) of the bodies of `subset`
int halo_pair_solve(xpbd_world *w, double h, uint32_t k, bool last, const BodySubset &subset)
{
    const BodyArrays b = w->arrays();
    const ContactBuffers c = w->contact_buffers(k & 1u);
    if (last)
        XPBD_HIP_TRY(launch_pair_solve_derive(b, b.dyn, h, c, w->stream, subset));
    else
        XPBD_HIP_TRY(launch_pair_solve_integrate_ground(b, w->shapes(), h, c, w->contact_buffers((k + 1u) & 1u).rec, w->last_mask.as<uint32_t>(),
                                                        nullptr, k + 1, w->stream, subset));
    return XPBD_OK;
}
} // namespace

int halo_substep_boundary(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept
{
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    if (int rc = narrowphase_contacts(w, w->arrays(), w->contact_buffers(k & 1u)))
        return rc;
    XPBD_HIP_TRY(launch_joint_extras(h, w->contact_buffers(k & 1u), w->stream)); // every record of substep k is complete, ghosts included
    BodySubset subset;
    subset.list = l.boundary;
    subset.count = l.n_boundary;
    subset.export_rows = l.send;
    return halo_pair_solve(w, h, k, last, subset);
}

int halo_substep_interior(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept
{
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    BodySubset subset;
    subset.skip = l.skip;
    return halo_pair_solve(w, h, k, last, subset);
}

int halo_substep_ghosts(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept
{
    if (w->n == 0 || l.n_ghosts == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const BodyArrays b = w->arrays();
    if (last) {
        XPBD_HIP_TRY(launch_import_dynamic(b, l.ghosts, l.ghost_rows, l.n_ghosts, l.recv, w->stream));
        return XPBD_OK;
    }
    BodySubset subset;
    subset.list = l.ghosts;
    subset.count = l.n_ghosts;
    subset.import_buf = l.recv;
    subset.import_rows = l.ghost_rows;
    XPBD_HIP_TRY(launch_integrate_ground(b, w->shapes(), h, w->contact_buffers((k + 1u) & 1u), w->last_mask.as<uint32_t>(), nullptr, k + 1, w->stream,
                                         subset));
    return XPBD_OK;
}

} // namespace xpbd

namespace {
// Do all bodies of a shape share their mass properties bit for bit?  (see stat_shared)  One more body of shape `sid`.
void absorb_stat_record(xpbd_world *w, const xpbd_rigid &body, uint32_t sid)
{
    double v[xpbd::kStatRecDoubles] = {};
    v[0] = body.inverse_mass;
    std::memcpy(v + 1, body.inverse_inertia, 9 * sizeof(double));
    std::memcpy(v + 10, body.center_of_mass, 3 * sizeof(double));
    double *slot = w->stat_shape_host.data() + (size_t)sid * xpbd::kStatRecDoubles;
    if (!w->stat_shape_seen[sid]) {
        std::memcpy(slot, v, sizeof v);
        w->stat_shape_seen[sid] = 1;
    } else if (std::memcmp(slot, v, sizeof v) != 0) {
        w->stat_shared = false;
    }
}

// Before n more bodies are absorbed.  start_over: the bodies before them are gone (an upload, the first bodies of an empty
// world); a changed shape count starts over too, with the property lost.
void reset_stat_records(xpbd_world *w, bool start_over, uint32_t n)
{
    if (start_over || w->stat_shape_seen.size() != w->n_shapes) {
        w->stat_shape_host.assign((size_t)w->n_shapes * xpbd::kStatRecDoubles, 0.0);
        w->stat_shape_seen.assign(w->n_shapes, 0);
        w->stat_shared = start_over && n != 0;
    }
}

constexpr uint32_t kMaxBodies = 0xFFFFFF00u; // the largest count whose stride fits 32 bits
uint32_t stride_for(uint32_t n_bodies) { return round_up(n_bodies ? n_bodies : 1, 256); }

// The body arrays hold n_new bodies from now on (the caller made room: stride_for(n_new)): what was derived from the old
// bodies is dropped -- neighbour lists, history, trace, contact masks, frame snapshot and the contact report's state.
void take_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id)
{
    w->have_neighbours = false;
    w->history_length = 0;
    w->history_stepped.clear();
    w->n = n_new;
    w->stride = stride_for(n_new);
    w->stat_rec_valid = false;
    w->max_shape_id = max_shape_id;
    w->stepped = false;
    w->trace_rows = 0;
    w->frame_snapshot_valid = false;
    w->bp_pending = false;
    report_reset(w);
}

// The settings that name bodies (or the joints between them) by index go back to their defaults.
void drop_body_settings(xpbd_world *w)
{
    w->joints.clear();
    w->filters.clear();
    w->materials.clear();
    w->restitution.clear();
}

// The world takes a new set of n_new bodies (xpbd_world_upload_bodies, xpbd::repack_bodies; device bound, stream idle): room for
// them, and everything that named the old bodies by index or was derived from them is dropped -- the body-indexed settings
// (drop_body_settings) and the derived state (take_body_count).  The callers fill the arrays and see to the per-shape mass
// properties (stat_shape_*), which one resets and the other keeps.  (A population change keeps the settings: it stages its
// arrays itself and calls take_body_count alone.)
int adopt_body_count(xpbd_world *w, uint32_t n_new, uint32_t max_shape_id)
{
    // (the stride rounds the count up to a multiple of 256; and no body index can then be XPBD_HIT_TERRAIN or XPBD_NO_HIT)
    static_assert(kMaxBodies - 1u < XPBD_HIT_TERRAIN && XPBD_HIT_TERRAIN < XPBD_NO_HIT, "the scene queries' reserved body indices are no body's");
    if (n_new > kMaxBodies)
        return set_error(XPBD_E_INVALID, "a world holds at most %u bodies, not %u", kMaxBodies, n_new);
    const uint32_t stride = stride_for(n_new);
    XPBD_HIP_TRY(w->dyn.reserve((size_t)xpbd::kDynFields * stride * 8));
    drop_body_settings(w);
    XPBD_HIP_TRY(w->stat.reserve((size_t)xpbd::kStatFields * stride * 8));
    XPBD_HIP_TRY(w->shape_id.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(w->last_mask.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(w->aos_staging.reserve((size_t)(n_new ? n_new : 1) * sizeof(xpbd_rigid)));
    take_body_count(w, n_new, max_shape_id);
    return XPBD_OK;
}

// `bytes` (> 0) of `values` in a block of its own.
int stage_upload(DeviceBuffer &fresh, const void *values, size_t bytes)
{
    XPBD_HIP_TRY(fresh.reserve(bytes));
    XPBD_HIP_TRY(hipMemcpy(fresh.ptr, values, bytes, hipMemcpyHostToDevice));
    return XPBD_OK;
}

// A per-body table of a setter: staged in a buffer of its own and moved over `table`, so that a failed allocation or copy
// leaves the previous table in force.  The stream is idle (queued work may still read the present table).
int upload_table(DeviceBuffer &table, const void *values, size_t bytes)
{
    DeviceBuffer fresh;
    XPBD_TRY(stage_upload(fresh, values, bytes));
    table = std::move(fresh);
    return XPBD_OK;
}

// ---- the joint tables (JointTables): nothing but these three allocates or copies one ----------------------------------------
// Each fills a fresh part from the host tables of xpbd_population_remap.hpp; the caller moves it in once nothing can fail any
// more, so a failed call leaves the previous tables in force.  An empty part is left without blocks, so every table that is
// copied has at least one element.  The device is bound.
int stage_csr(const xpbd_joint *joints, uint32_t n_joints, const xpbd::JointCsr &csr, uint32_t n_bodies, JointTables::Csr &out)
{
    static_assert(sizeof(xpbd_joint) == sizeof(xpbd::Joint), "xpbd_joint must mirror xpbd::Joint");
    if (n_joints == 0)
        return XPBD_OK;
    XPBD_TRY(stage_upload(out.joints, joints, (size_t)n_joints * sizeof(xpbd::Joint)));
    XPBD_TRY(stage_upload(out.off, csr.off.data(), (size_t)(n_bodies + 1) * 4));
    XPBD_TRY(stage_upload(out.list, csr.list.data(), (size_t)2 * n_joints * 4));
    out.n = n_joints;
    return XPBD_OK;
}

int stage_limits(const xpbd::LimitTables &t, JointTables::Limits &out)
{
    if (t.sorted.empty())
        return XPBD_OK;
    XPBD_TRY(stage_upload(out.limits, t.sorted.data(), t.sorted.size() * sizeof(xpbd::JointLimit)));
    XPBD_TRY(stage_upload(out.limit_off, t.off.data(), t.off.size() * 4));
    out.n_limits = (uint32_t)t.sorted.size();
    return XPBD_OK;
}

// The per-end sums start as zeros, which is what the pair solve reads for a joint that is not listed.
int stage_extras(const xpbd::ExtraTables &t, uint32_t n_joints, hipStream_t stream, JointTables::Extras &out)
{
    static_assert(xpbd::kExtraItemSlideLimit == xpbd::kExtraSlideLimit && sizeof(xpbd::ExtraItem) == sizeof(xpbd::JointExtraItem),
                  "xpbd::ExtraItem must mirror xpbd::JointExtraItem");
    if (t.list.empty())
        return XPBD_OK;
    const size_t sums = (size_t)2 * n_joints * xpbd::kJointExtraDoubles * 8;
    XPBD_HIP_TRY(out.sums.reserve(sums));
    XPBD_HIP_TRY(hipMemsetAsync(out.sums.ptr, 0, sums, stream));
    XPBD_HIP_TRY(hipStreamSynchronize(stream)); // done before the call returns: a stream the world is given later reads zeros too
    XPBD_TRY(stage_upload(out.joints, t.list.data(), t.list.size() * 4));
    XPBD_TRY(stage_upload(out.slots, t.slots.data(), t.slots.size() * 4));
    XPBD_TRY(stage_upload(out.off, t.off.data(), t.off.size() * 4));
    XPBD_TRY(stage_upload(out.items, t.items.data(), t.items.size() * sizeof(xpbd::ExtraItem)));
    out.n_extra_joints = (uint32_t)t.list.size();
    return XPBD_OK;
}

// All three from `set` in a world of n_bodies bodies: what the three setters, called in turn, would build.
int stage_joint_tables(xpbd::JointSet set, uint32_t n_bodies, hipStream_t stream, JointTables &out)
{
    out.clear();
    const uint32_t n_joints = (uint32_t)set.joints.size();
    if (n_joints == 0)
        return XPBD_OK;
    xpbd::LimitTables lt = xpbd::build_limit_tables(set.limits.data(), (uint32_t)set.limits.size(), n_joints);
    XPBD_TRY(stage_csr(set.joints.data(), n_joints, xpbd::build_joint_csr(set.joints.data(), n_joints, n_bodies), n_bodies, out.csr));
    XPBD_TRY(stage_limits(lt, out.limits));
    XPBD_TRY(stage_extras(xpbd::build_extra_tables(set.joints, lt.slide, set.drives, n_bodies), n_joints, stream, out.extras));
    out.set = std::move(set);
    out.slide_limits = std::move(lt.slide);
    return XPBD_OK;
}
} // namespace

// ---- re-planning a shard of the multi-GPU world on the device (xpbd_multi.cpp) ---------------------------------------------
namespace xpbd {

int halo_cell_keys(xpbd_world *w, const uint32_t *dev_slots, uint32_t n, double edge, int64_t *host_keys, uint32_t *bad_index)
{
    *bad_index = UINT32_MAX;
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() may free a block
    XPBD_HIP_TRY(w->halo_keys.reserve((size_t)n * 8 + 8));
    uint32_t *bad = reinterpret_cast<uint32_t *>(w->halo_keys.as<int64_t>() + n);
    XPBD_HIP_TRY(hipMemsetAsync(bad, 0xFF, 4, w->stream));
    XPBD_HIP_TRY(launch_cell_keys(w->arrays(), dev_slots, n, edge, w->halo_keys.as<int64_t>(), bad, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(host_keys, w->halo_keys.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(bad_index, bad, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

int download_records(xpbd_world *w, const uint32_t *host_slots, uint32_t n, double *out39)
{
    if (n == 0)
        return XPBD_OK;
    for (uint32_t k = 0; k < n; ++k)
        if (host_slots[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd::download_records: slot %u of a world of %u bodies", host_slots[k], w->n);
    if (int rc = bind_device(w))
        return rc;
    constexpr size_t rec = (size_t)(kRigidDoubles + 1) * 8;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->halo_records.reserve((size_t)n * rec));
    XPBD_HIP_TRY(w->repack_src.reserve((size_t)n * 4));
    XPBD_HIP_TRY(hipMemcpyAsync(w->repack_src.ptr, host_slots, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(launch_gather_records(w->arrays(), w->repack_src.as<uint32_t>(), n, w->halo_records.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out39, w->halo_records.ptr, (size_t)n * rec, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

// The world's bodies become: body s = the present body src[s] (src[s] >= 0) or incoming record -src[s] - 1 (39 doubles: an
// xpbd_rigid and its shape id).  Everything stays on the device but the incoming records; otherwise as xpbd_world_upload_bodies
// (joints, history, contact masks and the neighbour lists are dropped).
int repack_bodies(xpbd_world *w, const int32_t *host_src, uint32_t n_new, const double *incoming39, uint32_t n_incoming)
{
    if (!w || (n_new && !host_src) || (n_incoming && !incoming39))
        return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: NULL argument");
    constexpr uint32_t rec = kRigidDoubles + 1;
    uint32_t max_shape_id = w->max_shape_id;
    for (uint32_t s = 0; s < n_new; ++s) {
        const int32_t from = host_src[s];
        if (from >= 0 ? (uint32_t)from >= w->n : (uint32_t)(-(from + 1)) >= n_incoming)
            return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: body %u comes from %d (%u bodies present, %u incoming)", s, from, w->n, n_incoming);
    }
    for (uint32_t k = 0; k < n_incoming; ++k) {
        const double sid = incoming39[(size_t)k * rec + kRigidDoubles];
        if (!(sid >= 0.0) || sid >= (double)w->n_shapes)
            return set_error(XPBD_E_INVALID, "xpbd::repack_bodies: incoming record %u has shape id %g of %u", k, sid, w->n_shapes);
        max_shape_id = std::max(max_shape_id, (uint32_t)sid);
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    // 1. the present bodies in AoS, the new ones gathered from them and from the incoming records
    XPBD_HIP_TRY(w->aos_staging.reserve((size_t)std::max(w->n, 1u) * sizeof(xpbd_rigid)));
    XPBD_HIP_TRY(w->repack_aos.reserve((size_t)std::max(n_new, 1u) * sizeof(xpbd_rigid)));
    XPBD_HIP_TRY(w->repack_shape.reserve((size_t)std::max(n_new, 1u) * 4));
    XPBD_HIP_TRY(w->repack_src.reserve((size_t)std::max(n_new, 1u) * 4));
    XPBD_HIP_TRY(w->repack_incoming.reserve((size_t)std::max(n_incoming, 1u) * rec * 8));
    XPBD_HIP_TRY(launch_soa_to_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    if (n_new)
        XPBD_HIP_TRY(hipMemcpyAsync(w->repack_src.ptr, host_src, (size_t)n_new * 4, hipMemcpyHostToDevice, w->stream));
    if (n_incoming)
        XPBD_HIP_TRY(hipMemcpyAsync(w->repack_incoming.ptr, incoming39, (size_t)n_incoming * rec * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(launch_repack_bodies(w->aos_staging.as<double>(), w->shape_id.as<uint32_t>(), w->repack_src.as<int32_t>(), n_new,
                                      w->repack_incoming.as<double>(), w->repack_aos.as<double>(), w->repack_shape.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the arrays below may move
    // 2. the world takes the new size
    XPBD_TRY(adopt_body_count(w, n_new, max_shape_id));
    // mass properties shared per shape: the bodies that stay kept the property, the incoming ones are checked
    reset_stat_records(w, false, n_incoming);
    for (uint32_t k = 0; k < n_incoming && w->stat_shared; ++k) {
        xpbd_rigid body;
        std::memcpy(&body, incoming39 + (size_t)k * rec, sizeof body);
        absorb_stat_record(w, body, (uint32_t)incoming39[(size_t)k * rec + kRigidDoubles]);
    }
    if (n_new == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipMemsetAsync(w->shape_id.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->shape_id.ptr, w->repack_shape.ptr, (size_t)n_new * 4, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->last_mask.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(launch_aos_to_soa(w->repack_aos.as<double>(), w->arrays(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's buffers are only borrowed
    return XPBD_OK;
}

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

int check_joint_limits(const char *who, const xpbd_joint *joints, uint32_t n_joints, const xpbd_joint_limit *limits, uint32_t n_limits)
{
    static_assert(sizeof(xpbd_joint_limit) == 72 && sizeof(xpbd_joint_limit) == sizeof(JointLimit), "xpbd_joint_limit must mirror xpbd::JointLimit");
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
    static_assert(sizeof(xpbd_joint_drive) == 80 && sizeof(xpbd_joint_drive) == sizeof(JointExtraItem), "xpbd_joint_drive must mirror xpbd::JointExtraItem");
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

// The flags' part of the three checks: `known` are the family's own bits.
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

// The terrain a query with these flags asks about (null: none; the checks have refused the flag on a world without one).
const Terrain *query_terrain(const xpbd_world *w, uint32_t flags) { return (flags & XPBD_QUERY_TERRAIN) && w->terrain.planes ? &w->terrain : nullptr; }

// The filter table a masked query reads (null: unmasked, or no filters set -- every body is then in group ~0u).
const uint2 *masked_filter(const xpbd_world *w, bool masked) { return masked && w->filters.on ? w->ft_filters.as<uint2>() : nullptr; }

// The host variant of a query with one result per record: n records in, enqueue(device records, device results), n results out,
// and the stream synchronised.
template <class In, class Out, class Enqueue>
int query_host(xpbd_world *w, const In *in, uint32_t n, Out *out, Enqueue &&enqueue)
{
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    SceneQueryScratch &s = w->query;
    const size_t in_bytes = (size_t)n * sizeof(In), out_bytes = (size_t)n * sizeof(Out);
    XPBD_HIP_TRY(s.reserve(QuerySizes{}, in_bytes, out_bytes, 0, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(s.in.ptr, in, in_bytes, hipMemcpyHostToDevice, w->stream));
    if (int rc = enqueue(s.in.as<In>(), s.out.as<Out>()))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(out, s.out.ptr, out_bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
}

int raycast_enqueue(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *dev_hits,
                    const uint32_t *dev_global_id, bool masked, uint32_t mask)
{
    static_assert(sizeof(xpbd_ray) == 64 && sizeof(xpbd_ray_hit) == 64, "xpbd_ray and xpbd_ray_hit are 64 bytes");
    if (n_rays == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // (a world without bodies takes the brute-force path too: every ray misses, no grid to build)
    const bool brute = (flags & XPBD_RAYCAST_BRUTE_FORCE) || n_rays <= XPBD_RAYCAST_BRUTE_FORCE_RAYS || w->n == 0;
    const QuerySizes q = query_scratch_bytes(w->n, n_rays, brute);
    XPBD_HIP_TRY(w->query.reserve(q, 0, 0, 0, w->stream));
    const RayFilter filter{masked_filter(w, masked), mask, masked ? 1u : 0u};
    XPBD_HIP_TRY(launch_raycast(w->arrays(), w->tables(), dev_global_id, filter, dev_rays, n_rays, brute, w->query.view(q.table_size), dev_hits,
                                w->stream, query_terrain(w, flags), (flags & XPBD_RAYCAST_BRUTE_FORCE) != 0));
    return XPBD_OK;
}

int raycast_host(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits, const uint32_t *dev_global_id,
                 bool masked, uint32_t mask)
{
    return query_host(w, rays, n_rays, hits, [&](const xpbd_ray *dev_rays, xpbd_ray_hit *dev_hits) {
        return raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, dev_global_id, masked, mask);
    });
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

int overlap_enqueue(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags, uint32_t *dev_offsets,
                    xpbd_overlap_hit *dev_hits, uint32_t cap, const uint32_t *dev_global_id)
{
    static_assert(sizeof(xpbd_overlap_query) == 72 && sizeof(xpbd_overlap_hit) == 16, "xpbd_overlap_query is 72 bytes, xpbd_overlap_hit 16");
    if (int rc = bind_device(w))
        return rc;
    if (n_queries == 0) {
        if (dev_offsets)
            XPBD_HIP_TRY(hipMemsetAsync(dev_offsets, 0, sizeof(uint32_t), w->stream));
        return XPBD_OK;
    }
    const bool brute = (flags & XPBD_OVERLAP_BRUTE_FORCE) || w->n == 0;
    const QuerySizes q = overlap_scratch_bytes(w->n, n_queries, brute);
    XPBD_HIP_TRY(w->query.reserve(q, 0, 0, 0, w->stream));
    const bool masked = (flags & XPBD_OVERLAP_MASKED) != 0;
    XPBD_HIP_TRY(launch_overlap(w->arrays(), w->tables(), dev_global_id, masked_filter(w, masked), dev_queries, n_queries, masked, brute,
                                w->query.view(q.table_size), dev_offsets, dev_hits, cap, w->stream, query_terrain(w, flags)));
    return XPBD_OK;
}

int overlap_host(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets, xpbd_overlap_hit *hits,
                 uint32_t cap, uint32_t *n_out, const uint32_t *dev_global_id)
{
    *n_out = 0;
    if (n_queries == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    SceneQueryScratch &s = w->query;
    const size_t q_bytes = (size_t)n_queries * sizeof(xpbd_overlap_query), o_bytes = ((size_t)n_queries + 1) * sizeof(uint32_t);
    XPBD_HIP_TRY(s.reserve(QuerySizes{}, q_bytes, (size_t)(cap ? cap : 1) * sizeof(xpbd_overlap_hit), o_bytes, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(s.in.ptr, queries, q_bytes, hipMemcpyHostToDevice, w->stream));
    if (int rc = overlap_enqueue(w, s.in.as<xpbd_overlap_query>(), n_queries, flags, s.offsets.as<uint32_t>(),
                                 cap ? s.out.as<xpbd_overlap_hit>() : nullptr, cap, dev_global_id))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(offsets, s.offsets.ptr, o_bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = offsets[n_queries], held = total < cap ? total : cap;
    if (held) {
        XPBD_HIP_TRY(hipMemcpyAsync(hits, s.out.ptr, (size_t)held * sizeof(xpbd_overlap_hit), hipMemcpyDeviceToHost, w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    *n_out = total;
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "overlap query: %u hits but room for %u", total, cap);
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

int sweep_enqueue(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *dev_hits,
                  const uint32_t *dev_global_id)
{
    static_assert(sizeof(xpbd_sweep) == 104 && sizeof(xpbd_sweep_hit) == 72, "xpbd_sweep is 104 bytes, xpbd_sweep_hit 72");
    if (n_sweeps == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // (a shard without bodies takes the brute-force path too: every sweep misses, no grid to build)
    const bool brute = (flags & XPBD_SWEEP_BRUTE_FORCE) || n_sweeps <= XPBD_SWEEP_BRUTE_FORCE_SWEEPS || w->n == 0;
    const QuerySizes q = overlap_scratch_bytes(w->n, n_sweeps, brute); // a sweep's records are an overlap query's
    XPBD_HIP_TRY(w->query.reserve(q, 0, 0, 0, w->stream));
    const bool masked = (flags & XPBD_SWEEP_MASKED) != 0;
    XPBD_HIP_TRY(launch_sweep(w->arrays(), w->tables(), dev_global_id, masked_filter(w, masked), dev_sweeps, n_sweeps, masked, brute,
                              w->query.view(q.table_size), dev_hits, w->stream, query_terrain(w, flags), (flags & XPBD_SWEEP_BRUTE_FORCE) != 0));
    return XPBD_OK;
}

int sweep_host(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits, const uint32_t *dev_global_id)
{
    return query_host(w, sweeps, n_sweeps, hits, [&](const xpbd_sweep *dev_sweeps, xpbd_sweep_hit *dev_hits) {
        return sweep_enqueue(w, dev_sweeps, n_sweeps, flags, dev_hits, dev_global_id);
    });
}

} // namespace xpbd

extern "C" {

uint32_t xpbd_abi_version(void) noexcept { return XPBD_ABI_VERSION; }

void xpbd_config_default(xpbd_config *cfg) noexcept
{
    if (!cfg)
        return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0;
    cfg->mode = XPBD_MODE_FUSED;
}

int xpbd_device_count(void)
try {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
        return set_error(XPBD_E_NO_DEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    return n;
} XPBD_ABI_CATCH

int xpbd_world_create(xpbd_world **out, const xpbd_config *cfg)
try {
    if (!out)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: out is NULL");
    *out = nullptr;
    xpbd_config c;
    xpbd_config_default(&c);
    if (cfg) {
        if (cfg->struct_size != sizeof(xpbd_config))
            return set_error(XPBD_E_INVALID, "xpbd_world_create: struct_size %u != %zu", cfg->struct_size,
                             sizeof(xpbd_config));
        c = *cfg;
    }
    if (c.mode != XPBD_MODE_FUSED && c.mode != XPBD_MODE_PER_SUBSTEP && c.mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: unknown mode %u", c.mode);
    if (c.flags & ~XPBD_FLAG_TRACE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: unknown flags 0x%x", c.flags);
    // k_step is compiled with __launch_bounds__(xpbd::kMaxStepBlock): a larger workgroup is a launch failure
    if (c.block_size != 0 && (c.block_size % 64 != 0 || c.block_size > xpbd::kMaxStepBlock))
        return set_error(XPBD_E_INVALID, "xpbd_world_create: block_size %u must be a multiple of 64, <= %u",
                         c.block_size, xpbd::kMaxStepBlock);
    if (c.reserved[0] || c.reserved[1] || c.reserved[2])
        return set_error(XPBD_E_INVALID, "xpbd_world_create: reserved fields must be 0");

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return set_error(XPBD_E_NO_DEVICE, "no HIP device available (%s)",
                         e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (c.device < 0 || c.device >= count)
        return set_error(XPBD_E_INVALID, "xpbd_world_create: device %d out of range [0,%d)", c.device, count);

    std::unique_ptr<xpbd_world> w(new xpbd_world);
    w->device = c.device;
    w->mode = c.mode;
    w->flags = c.flags;
    w->block_size = c.block_size ? c.block_size : kDefaultBlock;
    e = hipSetDevice(w->device);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&w->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess)
        return set_error(XPBD_E_HIP, "xpbd_world_create: stream creation failed: %s", hipGetErrorString(e));
    w->stream = w->own_stream;
    *out = w.release();
    return XPBD_OK;
} XPBD_ABI_CATCH

void xpbd_world_destroy(xpbd_world *w) noexcept { delete w; }

int xpbd_world_set_shapes(xpbd_world *w, const double *verts_xyz, const uint32_t *vert_offsets,
                          uint32_t n_shapes)
try {
    if (!w || !verts_xyz || !vert_offsets || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: NULL argument or no shapes");
    if (vert_offsets[0] != 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: vert_offsets[0] must be 0");
    for (uint32_t s = 0; s < n_shapes; ++s) {
        if (vert_offsets[s + 1] < vert_offsets[s])
            return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: vert_offsets not monotone at %u", s);
        if (vert_offsets[s + 1] - vert_offsets[s] > XPBD_MAX_SHAPE_VERTS)
            return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: shape %u has %u vertices (max %u)", s,
                             vert_offsets[s + 1] - vert_offsets[s], XPBD_MAX_SHAPE_VERTS);
    }
    const uint32_t total = vert_offsets[n_shapes];
    // The tables are staged into LDS by every block; keep them far below the 160 KiB/CU.
    if ((size_t)total * 24 + (size_t)(n_shapes + 1) * 4 > 48 * 1024)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: shape tables exceed 48 KiB");
    // the resident bodies keep their shape ids: the kernels index the staged table with them unchecked
    if (w->n && n_shapes <= w->max_shape_id)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: %u shapes, but the uploaded bodies use shape id %u (upload bodies "
                                         "again after shrinking the table)", n_shapes, w->max_shape_id);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->shape_verts.reserve(total ? (size_t)total * 24 : 8));
    XPBD_HIP_TRY(w->shape_offsets.reserve((size_t)(n_shapes + 1) * 4));
    if (total)
        XPBD_HIP_TRY(hipMemcpy(w->shape_verts.ptr, verts_xyz, (size_t)total * 24, hipMemcpyHostToDevice));
    XPBD_HIP_TRY(hipMemcpy(w->shape_offsets.ptr, vert_offsets, (size_t)(n_shapes + 1) * 4, hipMemcpyHostToDevice));
    w->n_shapes = n_shapes;
    w->total_verts = total;
    w->has_topology = false;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_polytopes(xpbd_world *w, const xpbd_polytope *shapes, uint32_t n_shapes)
try {
    if (!w || !shapes || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: NULL argument or no shapes");
    std::vector<double> verts, planes, centroids, radii, dirs;
    std::vector<uint32_t> vert_offsets{0}, face_start{0}, face_verts, edges, dir_id;
    std::vector<xpbd::ShapeDesc> desc;
    for (uint32_t s = 0; s < n_shapes; ++s) {
        const xpbd_polytope &p = shapes[s];
        if ((p.n_vertices && !p.vertices_xyz) || (p.n_edges && !p.edges) ||
            (p.n_faces && (!p.face_offsets || !p.face_indices)))
            return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: shape %u has a NULL table", s);
        if (p.n_vertices > XPBD_MAX_SHAPE_VERTS || p.n_faces > 64 || p.n_edges > 4096)
            return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: shape %u too large (%u vertices, %u faces, %u edges)",
                             s, p.n_vertices, p.n_faces, p.n_edges);
        xpbd::ShapeDesc d{};
        d.vert0 = (uint32_t)(verts.size() / 3);
        d.n_verts = p.n_vertices;
        d.face0 = (uint32_t)(planes.size() / 4);
        d.n_faces = p.n_faces;
        d.edge0 = (uint32_t)(edges.size() / 2);
        d.n_edges = p.n_edges;
        verts.insert(verts.end(), p.vertices_xyz, p.vertices_xyz + 3 * (size_t)p.n_vertices);
        vert_offsets.push_back((uint32_t)(verts.size() / 3));
        auto vertex = [&](uint32_t i) {
            return xpbd::Vec3{p.vertices_xyz[3 * i], p.vertices_xyz[3 * i + 1], p.vertices_xyz[3 * i + 2]};
        };
        for (uint32_t e = 0; e < 2 * p.n_edges; ++e) {
            if (p.edges[e] >= p.n_vertices)
                return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: shape %u edge vertex out of range", s);
            edges.push_back(p.edges[e]);
        }
        // unique edge directions (up to sign), first edge with a direction represents it
        d.dir0 = (uint32_t)(dirs.size() / 3);
        for (uint32_t e = 0; e < p.n_edges; ++e) {
            const xpbd::Vec3 dv = vertex(p.edges[2 * e + 1]) - vertex(p.edges[2 * e]);
            const uint32_t nd = (uint32_t)(dirs.size() / 3) - d.dir0;
            uint32_t found = nd;
            for (uint32_t k = 0; k < nd; ++k) {
                const double *u = &dirs[3 * (size_t)(d.dir0 + k)];
                const xpbd::Vec3 uv{u[0], u[1], u[2]};
                const xpbd::Vec3 c = xpbd::cross(dv, uv);
                if (xpbd::dot(c, c) <= 1e-12 * (xpbd::dot(dv, dv) * xpbd::dot(uv, uv))) {
                    found = k;
                    break;
                }
            }
            if (found == nd)
                dirs.insert(dirs.end(), {dv.x, dv.y, dv.z});
            dir_id.push_back(found);
        }
        d.n_dirs = (uint32_t)(dirs.size() / 3) - d.dir0;
        const xpbd::Vec3 centroid{p.centroid[0], p.centroid[1], p.centroid[2]};
        for (uint32_t f = 0; f < p.n_faces; ++f) {
            const uint32_t f0 = p.face_offsets[f], f1 = p.face_offsets[f + 1];
            if (f1 < f0 || f1 - f0 < 3 || f1 - f0 > xpbd::kMaxFaceVerts)
                return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: shape %u face %u needs 3..%u vertices", s, f,
                                 xpbd::kMaxFaceVerts);
            for (uint32_t q = f0; q < f1; ++q) {
                if (p.face_indices[q] >= p.n_vertices)
                    return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: shape %u face vertex out of range", s);
                face_verts.push_back(p.face_indices[q]);
            }
            face_start.push_back((uint32_t)face_verts.size());
            // Polytope::plane (src/geometry.rs:262-271) over Plane::from_points / facing / flip (:16-24, :55-68)
            const xpbd::Vec3 p0 = vertex(p.face_indices[f0]), p1 = vertex(p.face_indices[f0 + 1]),
                             p2 = vertex(p.face_indices[f0 + 2]);
            xpbd::Vec3 n = xpbd::normalized(xpbd::cross(p1 - p0, p2 - p0));
            double disp = xpbd::dot(n, p0);
            const bool facing = xpbd::dot(n, centroid - disp * n) >= 0.0;
            if (facing) {
                n = -n;
                disp = -disp;
            }
            planes.insert(planes.end(), {n.x, n.y, n.z, disp});
        }
        centroids.insert(centroids.end(), {centroid.x, centroid.y, centroid.z});
        double radius = 0.0; // bounding sphere about the centroid
        for (uint32_t k = 0; k < p.n_vertices; ++k) {
            const double dist = xpbd::length(vertex(k) - centroid);
            if (dist > radius)
                radius = dist;
        }
        radii.push_back(radius);
        desc.push_back(d);
    }
    static const double zero3[3] = {0, 0, 0};
    if (int rc = xpbd_world_set_shapes(w, verts.empty() ? zero3 : verts.data(), vert_offsets.data(), n_shapes))
        return rc;
    auto upload = [&](DeviceBuffer &buf, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = buf.reserve(bytes ? bytes : 8);
        if (e == hipSuccess && bytes)
            e = hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    XPBD_HIP_TRY(upload(w->planes, planes.data(), planes.size() * 8));
    XPBD_HIP_TRY(upload(w->centroids, centroids.data(), centroids.size() * 8));
    XPBD_HIP_TRY(upload(w->shape_desc, desc.data(), desc.size() * sizeof(xpbd::ShapeDesc)));
    XPBD_HIP_TRY(upload(w->face_start, face_start.data(), face_start.size() * 4));
    XPBD_HIP_TRY(upload(w->face_verts, face_verts.data(), face_verts.size() * 4));
    XPBD_HIP_TRY(upload(w->edges, edges.data(), edges.size() * 4));
    XPBD_HIP_TRY(upload(w->shape_radii, radii.data(), radii.size() * 8));
    XPBD_HIP_TRY(upload(w->edge_dirs, dirs.data(), dirs.size() * 8));
    XPBD_HIP_TRY(upload(w->edge_dir_id, dir_id.data(), dir_id.size() * 4));
    w->has_topology = true;
    uint32_t max_verts = 0, max_faces = 0, max_face_verts = 0, small_max_face_verts = 0, n_small = 0;
    std::vector<uint8_t> shape_class(n_shapes, 0);
    for (uint32_t k = 0; k < n_shapes; ++k) {
        max_verts = shapes[k].n_vertices > max_verts ? shapes[k].n_vertices : max_verts;
        max_faces = shapes[k].n_faces > max_faces ? shapes[k].n_faces : max_faces;
        const bool small = shapes[k].n_vertices <= 8 && shapes[k].n_faces <= 8;
        shape_class[k] = small ? 0 : 1;
        n_small += small;
        for (uint32_t f = 0; f < shapes[k].n_faces; ++f) {
            const uint32_t nfv = shapes[k].face_offsets[f + 1] - shapes[k].face_offsets[f];
            max_face_verts = nfv > max_face_verts ? nfv : max_face_verts;
            if (small)
                small_max_face_verts = nfv > small_max_face_verts ? nfv : small_max_face_verts;
        }
    }
    XPBD_HIP_TRY(upload(w->shape_class, shape_class.data(), shape_class.size()));
    w->two_classes = (n_small != 0 && n_small != n_shapes) ? 1u : 0u;
    w->small_max_face_verts = small_max_face_verts;
    w->max_verts = max_verts;
    w->max_faces = max_faces;
    w->max_face_verts = max_face_verts;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_narrowphase(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_manifold *out)
try {
    static_assert(sizeof(xpbd_manifold) == sizeof(xpbd::Manifold), "xpbd_manifold must mirror xpbd::Manifold");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: NULL argument");
    if (!w->has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->pair_buf.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->manifold_buf.reserve((size_t)n_pairs * sizeof(xpbd::Manifold)));
    XPBD_HIP_TRY(hipMemcpyAsync(w->pair_buf.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->manifold_buf.ptr, 0, (size_t)n_pairs * sizeof(xpbd::Manifold), w->stream));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_sat_pairs(w->arrays(), w->tables(), w->cb_rec.as<double>(), w->pair_buf.as<uint32_t>(),
                                        n_pairs, w->manifold_buf.as<xpbd::Manifold>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->manifold_buf.ptr, (size_t)n_pairs * sizeof(xpbd::Manifold),
                                hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_edge_axes_separation(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_edge_query *out)
try {
    static_assert(sizeof(xpbd_edge_query) == sizeof(xpbd::EdgeQuery), "xpbd_edge_query must mirror xpbd::EdgeQuery");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: NULL argument");
    if (!w->has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->pair_buf.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->manifold_buf.reserve((size_t)n_pairs * sizeof(xpbd::EdgeQuery)));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(hipMemcpyAsync(w->pair_buf.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_edge_axes_reference(w->arrays(), w->tables(), w->cb_rec.as<double>(), w->pair_buf.as<uint32_t>(), n_pairs,
                                                  w->manifold_buf.as<xpbd::EdgeQuery>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->manifold_buf.ptr, (size_t)n_pairs * sizeof(xpbd::EdgeQuery), hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_upload_bodies(xpbd_world *w, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n)
try {
    if (!w || (!aos && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: NULL argument");
    if (w->n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: call xpbd_world_set_shapes first");
    uint32_t max_shape_id = 0;
    if (shape_id)
        for (uint32_t i = 0; i < n; ++i) {
            if (shape_id[i] >= w->n_shapes)
                return set_error(XPBD_E_INVALID, "xpbd_world_upload_bodies: shape_id[%u] = %u >= n_shapes %u", i,
                                 shape_id[i], w->n_shapes);
            max_shape_id = shape_id[i] > max_shape_id ? shape_id[i] : max_shape_id;
        }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_TRY(adopt_body_count(w, n, max_shape_id));
    reset_stat_records(w, true, n);
    for (uint32_t i = 0; i < n && w->stat_shared; ++i)
        absorb_stat_record(w, aos[i], shape_id ? shape_id[i] : 0u);
    if (n == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipMemcpyAsync(w->aos_staging.ptr, aos, (size_t)n * sizeof(xpbd_rigid), hipMemcpyHostToDevice,
                                w->stream));
    if (shape_id)
        XPBD_HIP_TRY(hipMemcpyAsync(w->shape_id.ptr, shape_id, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    else
        XPBD_HIP_TRY(hipMemsetAsync(w->shape_id.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->last_mask.ptr, 0, (size_t)w->stride * 4, w->stream));
    XPBD_HIP_TRY(xpbd::launch_aos_to_soa(w->aos_staging.as<double>(), w->arrays(), w->stream));
    // The caller's buffers are only borrowed for the duration of the call.
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_bodies(xpbd_world *w, xpbd_rigid *aos, uint32_t n)
try {
    if (!w || (!aos && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_bodies: NULL argument");
    if (n != w->n)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_bodies: n = %u but the world holds %u bodies", n, w->n);
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_soa_to_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(aos, w->aos_staging.ptr, (size_t)n * sizeof(xpbd_rigid), hipMemcpyDeviceToHost,
                                w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_body_count(const xpbd_world *w) noexcept { return w ? w->n : 0; }

int xpbd_world_download_frames(xpbd_world *w, double *frames, uint32_t n)
try {
    if (!w || (!frames && n))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_frames: NULL argument");
    if (n != w->n)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_frames: n = %u but the world holds %u bodies", n, w->n);
    if (n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    // aos_staging holds n * 38 doubles: room for the n * 7 frame doubles
    XPBD_HIP_TRY(xpbd::launch_body_frames_aos(w->arrays(), w->aos_staging.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(frames, w->aos_staging.ptr, (size_t)n * 7 * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_step(xpbd_world *w, double dt, uint32_t substeps)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_step: NULL world");
    if (substeps == 0) // the reference divides by zero and runs no substep; treat as an argument error
        return set_error(XPBD_E_INVALID, "xpbd_world_step: substeps must be > 0");
    if (w->n_shapes == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_step: no shapes set");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const double h = dt / (double)substeps; // src/solver.rs:4
    uint32_t *trace = nullptr;
    if (w->flags & XPBD_FLAG_TRACE_CONTACTS) {
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() may free the previous buffer
        XPBD_HIP_TRY(w->trace.reserve((size_t)substeps * w->stride * 4));
        trace = w->trace.as<uint32_t>();
        w->trace_rows = substeps;
    }
    if (w->mode == XPBD_MODE_CONTACTS) {
        if (int rc = step_contacts(w, dt, h, substeps, trace)) {
            report_reset(w);
            return rc;
        }
    } else if (w->mode == XPBD_MODE_FUSED) {
        report_reset(w);
        XPBD_HIP_TRY(xpbd::launch_step(w->arrays(), w->shapes(), h, substeps, w->last_mask.as<uint32_t>(), trace, 0,
                                       w->block_size, w->stream));
    } else {
        report_reset(w);
        for (uint32_t k = 0; k < substeps; ++k)
            XPBD_HIP_TRY(xpbd::launch_step(w->arrays(), w->shapes(), h, 1, w->last_mask.as<uint32_t>(), trace, k,
                                           w->block_size, w->stream));
    }
    w->stepped = true;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_synchronize(xpbd_world *w)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_synchronize: NULL world");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_contacts(xpbd_world *w, xpbd_contact *out, uint32_t cap, uint32_t *n_out)
try {
    if (!w || !n_out || (!out && cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contacts: NULL argument");
    *n_out = 0;
    if (w->n == 0 || !w->stepped)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const uint32_t nb = (w->n + 255) / 256;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->block_counts.reserve((size_t)(nb + 1) * 4));
    XPBD_HIP_TRY(xpbd::launch_contacts_count(w->last_mask.as<uint32_t>(), w->n, w->block_counts.as<uint32_t>(),
                                             w->stream));
    uint32_t total = 0;
    XPBD_HIP_TRY(hipMemcpyAsync(&total, w->block_counts.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    *n_out = total;
    const uint32_t take = total < cap ? total : cap;
    if (take) {
        XPBD_HIP_TRY(w->contacts.reserve((size_t)take * sizeof(xpbd_contact)));
        XPBD_HIP_TRY(xpbd::launch_contacts_emit(w->last_mask.as<uint32_t>(), w->n, w->block_counts.as<uint32_t>(),
                                                w->contacts.as<xpbd_contact>(), take, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(out, w->contacts.ptr, (size_t)take * sizeof(xpbd_contact), hipMemcpyDeviceToHost,
                                    w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_contacts: %u contacts, capacity %u", total, cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_contact_masks(xpbd_world *w, uint32_t *masks, uint32_t substeps, uint32_t n)
try {
    if (!w || !masks)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: NULL argument");
    if (!(w->flags & XPBD_FLAG_TRACE_CONTACTS))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: world created without "
                                         "XPBD_FLAG_TRACE_CONTACTS");
    if (n != w->n || substeps != w->trace_rows)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_masks: asked for %u x %u, last step recorded %u x %u",
                         substeps, n, w->trace_rows, w->n);
    if (n == 0 || substeps == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipMemcpy2DAsync(masks, (size_t)n * 4, w->trace.ptr, (size_t)w->stride * 4, (size_t)n * 4, substeps,
                                  hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_stream(xpbd_world *w, void *hip_stream)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_stream: NULL world");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    w->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : w->own_stream;
    return XPBD_OK;
} XPBD_ABI_CATCH

void *xpbd_world_get_stream(const xpbd_world *w) noexcept { return w ? static_cast<void *>(w->stream) : nullptr; }

int xpbd_world_set_mode(xpbd_world *w, uint32_t mode)
try {
    if (!w || (mode != XPBD_MODE_FUSED && mode != XPBD_MODE_PER_SUBSTEP && mode != XPBD_MODE_CONTACTS))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_mode: bad argument");
    w->mode = mode;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_step_one(xpbd_rigid *rigid, const double *verts_xyz, uint32_t nverts, double dt, uint32_t substeps)
try {
    if (!rigid || !verts_xyz)
        return set_error(XPBD_E_INVALID, "xpbd_step_one: NULL argument");
    // One cached single-body world per host thread (the reference's step is re-entrant and
    // stateless; so is this apart from the cache).
    struct Cache {
        xpbd_world *w = nullptr;
        ~Cache() { xpbd_world_destroy(w); }
    };
    thread_local Cache cache;
    if (!cache.w) {
        xpbd_config cfg;
        xpbd_config_default(&cfg);
        if (int rc = xpbd_world_create(&cache.w, &cfg))
            return rc;
    }
    const uint32_t offsets[2] = {0, nverts};
    if (int rc = xpbd_world_set_shapes(cache.w, verts_xyz, offsets, 1))
        return rc;
    if (int rc = xpbd_world_upload_bodies(cache.w, rigid, nullptr, 1))
        return rc;
    if (int rc = xpbd_world_step(cache.w, dt, substeps))
        return rc;
    return xpbd_world_download_bodies(cache.w, rigid, 1);
} XPBD_ABI_CATCH

int xpbd_world_narrowphase_gjk(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_gjk_result *out)
try {
    static_assert(sizeof(xpbd_gjk_result) == sizeof(xpbd::GjkResult), "xpbd_gjk_result must mirror xpbd::GjkResult");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: NULL argument");
    if (!w->has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->pair_buf.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->manifold_buf.reserve((size_t)n_pairs * sizeof(xpbd::GjkResult)));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(hipMemcpyAsync(w->pair_buf.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->manifold_buf.ptr, 0, (size_t)n_pairs * sizeof(xpbd::GjkResult), w->stream));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    if (int rc = ensure_gjk_scratch(w, n_pairs))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_gjk_epa_pairs(w->arrays(), w->tables(), w->cb_rec.as<double>(),
                                            w->pair_buf.as<uint32_t>(), n_pairs, w->manifold_buf.as<xpbd::GjkResult>(),
                                            nullptr, w->gjk_scratch, false, nullptr, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->manifold_buf.ptr, (size_t)n_pairs * sizeof(xpbd::GjkResult), hipMemcpyDeviceToHost,
                                w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

// The three joint setters: validate, stage the affected parts aside (stage_csr / stage_limits / stage_extras), then commit by
// moves that cannot fail.  Queued substeps may still read the present tables: the stream is waited for first.
int xpbd_world_set_joints(xpbd_world *w, const xpbd_joint *joints, uint32_t n_joints)
try {
    if (!w || (n_joints && !joints))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joints: NULL argument");
    if (n_joints && w->mode != XPBD_MODE_CONTACTS) // only the contact pipeline projects joints: do not accept and ignore them
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joints: joints need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    XPBD_TRY(xpbd::check_joints("xpbd_world_set_joints", joints, n_joints, w->n));
    xpbd::JointSet set; // (limits and drives name joints by index: new joints drop them)
    set.joints.assign(joints, joints + n_joints);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables fresh;
    XPBD_TRY(stage_joint_tables(std::move(set), w->n, w->stream, fresh)); // (a slider has an extra entry of its own; no joints: all empty)
    w->joints = std::move(fresh);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_joint_limits(xpbd_world *w, const xpbd_joint_limit *limits, uint32_t n_limits)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_limits: NULL world");
    if (n_limits && w->mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_limits: limits need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    JointTables &J = w->joints;
    XPBD_TRY(xpbd::check_joint_limits("xpbd_world_set_joint_limits", J.set.joints.data(), J.csr.n, limits, n_limits));
    // the SLIDE limits apart (entries of k_joint_extras), the angular ones behind a CSR joint -> limits
    std::vector<xpbd_joint_limit> all(limits, limits + n_limits);
    xpbd::LimitTables lt = xpbd::build_limit_tables(limits, n_limits, J.csr.n);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables::Limits fresh;
    XPBD_TRY(stage_limits(lt, fresh));
    const bool slide_changes = !lt.slide.empty() || !J.slide_limits.empty();
    JointTables::Extras extras;
    if (slide_changes)
        XPBD_TRY(stage_extras(xpbd::build_extra_tables(J.set.joints, lt.slide, J.set.drives, w->n), J.csr.n, w->stream, extras));
    J.set.limits = std::move(all);
    J.slide_limits = std::move(lt.slide);
    J.limits = std::move(fresh);
    if (slide_changes)
        J.extras = std::move(extras);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_joint_drives(xpbd_world *w, const xpbd_joint_drive *drives, uint32_t n_drives)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_drives: NULL world");
    if (n_drives && w->mode != XPBD_MODE_CONTACTS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_joint_drives: drives need XPBD_MODE_CONTACTS (world is in mode %u)", w->mode);
    JointTables &J = w->joints;
    XPBD_TRY(xpbd::check_joint_drives("xpbd_world_set_joint_drives", J.set.joints.data(), J.csr.n, drives, n_drives));
    if (n_drives == 0 && J.set.drives.empty())
        return XPBD_OK;
    std::vector<xpbd_joint_drive> all(drives, drives + n_drives);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    JointTables::Extras fresh;
    XPBD_TRY(stage_extras(xpbd::build_extra_tables(J.set.joints, J.slide_limits, all, w->n), J.csr.n, w->stream, fresh));
    J.set.drives = std::move(all);
    J.extras = std::move(fresh);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_collision_filters(xpbd_world *w, const xpbd_collision_filter *filters, uint32_t n, uint32_t flags)
try {
    static_assert(sizeof(xpbd_collision_filter) == sizeof(uint2), "xpbd_collision_filter must mirror uint2 {group, mask}");
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_collision_filters: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_collision_filters", "filters", filters, n, w->n));
    if (flags & ~XPBD_FILTER_JOINTED)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_collision_filters: unknown flags 0x%x", flags);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued broadphases may still read the present filters
    if (!filters || n == 0) {
        w->filters.clear();
        w->filters.flags = flags;
        return XPBD_OK;
    }
    XPBD_TRY(upload_table(w->ft_filters, filters, (size_t)n * sizeof(uint2)));
    w->filters.on = true;
    w->filters.flags = flags;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_materials(xpbd_world *w, const xpbd_material *materials, uint32_t n, double ground_friction)
try {
    static_assert(sizeof(xpbd_material) == 16, "xpbd_material is {friction, reserved}");
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_materials: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_materials", "materials", materials, n, w->n));
    if (!(ground_friction >= 0.0))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_materials: ground_friction = %g (must be >= 0, +inf allowed)", ground_friction);
    if (int rc = xpbd::check_materials("xpbd_world_set_materials", materials, n))
        return rc;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present coefficients
    const double inf = std::numeric_limits<double>::infinity();
    if ((!materials || n == 0) && ground_friction == inf) { // the default: the contact kernels' plain forms
        w->materials.clear();
        return XPBD_OK;
    }
    // (a finite ground coefficient alone: every body +inf, so that the kernels have one switch, the array)
    std::vector<double> friction(std::max(w->n, 1u), inf);
    for (uint32_t i = 0; materials && i < n; ++i)
        friction[i] = materials[i].friction;
    XPBD_TRY(upload_table(w->mt_friction, friction.data(), friction.size() * sizeof(double)));
    w->materials.on = true;
    w->materials.ground_friction = ground_friction;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_restitution(xpbd_world *w, const double *restitution, uint32_t n, double ground_restitution, double bounce_threshold)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: NULL world");
    XPBD_TRY(xpbd::check_per_body("xpbd_world_set_restitution", "restitution", restitution, n, w->n));
    if (!(ground_restitution >= 0.0 && ground_restitution <= 1.0))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: ground_restitution = %g (must be in [0, 1])", ground_restitution);
    if (!(bounce_threshold >= 0.0 && bounce_threshold <= std::numeric_limits<double>::max()))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: bounce_threshold = %g (must be >= 0 and finite)", bounce_threshold);
    bool any = ground_restitution > 0.0;
    for (uint32_t i = 0; restitution && i < n; ++i) {
        if (!(restitution[i] >= 0.0 && restitution[i] <= 1.0))
            return set_error(XPBD_E_INVALID, "xpbd_world_set_restitution: restitution[%u] = %g (must be in [0, 1])", i, restitution[i]);
        any = any || restitution[i] > 0.0;
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present coefficients
    if (!any) { // nothing can bounce: the step runs what it ran before the call
        w->restitution.clear();
        w->restitution.bounce_threshold = bounce_threshold;
        return XPBD_OK;
    }
    std::vector<double> values(std::max(w->n, 1u), 0.0);
    for (uint32_t i = 0; restitution && i < n; ++i)
        values[i] = restitution[i];
    const uint32_t stride = w->stride ? w->stride : 256u;
    XPBD_HIP_TRY(w->dyn_alt.reserve((size_t)xpbd::kDynFields * stride * 8));
    XPBD_HIP_TRY(w->rs_start.reserve((size_t)6 * stride * 8));
    XPBD_TRY(upload_table(w->rs_restitution, values.data(), values.size() * sizeof(double)));
    w->restitution.on = true;
    w->restitution.ground = ground_restitution;
    w->restitution.bounce_threshold = bounce_threshold;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_terrain(xpbd_world *w, const xpbd_heightfield *hf)
try {
    static_assert(sizeof(xpbd_heightfield) == 48, "xpbd_heightfield is {nx, ny, origin[2], cell[2], heights}");
    const char *who = "xpbd_world_set_terrain";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    size_t samples = 0;
    if (hf) {
        if (hf->nx < 2 || hf->ny < 2)
            return set_error(XPBD_E_INVALID, "%s: %u x %u samples (each must be >= 2)", who, hf->nx, hf->ny);
        samples = (size_t)hf->nx * hf->ny;
        if (samples > XPBD_MAX_TERRAIN_SAMPLES)
            return set_error(XPBD_E_INVALID, "%s: %u x %u samples (at most %u)", who, hf->nx, hf->ny, XPBD_MAX_TERRAIN_SAMPLES);
        if (!hf->heights)
            return set_error(XPBD_E_INVALID, "%s: NULL heights", who);
        for (int a = 0; a < 2; ++a) {
            if (!std::isfinite(hf->origin[a]))
                return set_error(XPBD_E_INVALID, "%s: origin[%d] = %g (must be finite)", who, a, hf->origin[a]);
            if (!(std::isfinite(hf->cell[a]) && hf->cell[a] > 0.0))
                return set_error(XPBD_E_INVALID, "%s: cell[%d] = %g (must be finite and > 0)", who, a, hf->cell[a]);
        }
        for (size_t k = 0; k < samples; ++k)
            if (!std::isfinite(hf->heights[k]))
                return set_error(XPBD_E_INVALID, "%s: heights[%zu] = %g (must be finite)", who, k, hf->heights[k]);
    }
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present table
    if (!hf) {
        w->terrain = xpbd::Terrain{};
        w->tr_planes.release();
        return XPBD_OK;
    }
    // heights and the new table in blocks of their own: the present table stays in force until nothing can fail any more
    xpbd::Terrain t{nullptr, hf->origin[0], hf->origin[1], hf->cell[0], hf->cell[1], hf->nx, hf->ny};
    DeviceBuffer heights, planes;
    XPBD_TRY(stage_upload(heights, hf->heights, samples * sizeof(double)));
    XPBD_HIP_TRY(planes.reserve((size_t)(hf->nx - 1) * (hf->ny - 1) * 8 * sizeof(double)));
    XPBD_HIP_TRY(xpbd::launch_terrain_planes(heights.as<double>(), t, planes.as<double>(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    w->tr_planes = std::move(planes);
    t.planes = w->tr_planes.as<double>();
    w->terrain = t;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_sample_terrain(xpbd_world *w, const double *xy, uint32_t n, double *height, double *normal_xyz)
try {
    const char *who = "xpbd_world_sample_terrain";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (!w->terrain.planes)
        return set_error(XPBD_E_INVALID, "%s: the world has no terrain (xpbd_world_set_terrain)", who);
    if (n == 0)
        return XPBD_OK;
    if (!xy || !height)
        return set_error(XPBD_E_INVALID, "%s: NULL xy or height", who);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->tr_xy, (size_t)n * 2 * 8}, {w->tr_out, (size_t)n * 4 * 8}}));
    double *dev_height = w->tr_out.as<double>(), *dev_normal = normal_xyz ? dev_height + n : nullptr;
    XPBD_HIP_TRY(hipMemcpyAsync(w->tr_xy.ptr, xy, (size_t)n * 2 * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_sample_terrain(w->terrain, w->tr_xy.as<double>(), n, dev_height, dev_normal, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(height, dev_height, (size_t)n * 8, hipMemcpyDeviceToHost, w->stream));
    if (normal_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(normal_xyz, dev_normal, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_contacts_begin(xpbd_world *w, double dt)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: NULL world");
    if (w->mode != XPBD_MODE_CONTACTS || !w->has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (int rc = bind_device(w))
        return rc;
    w->stepped = true;
    if (w->n == 0)
        return XPBD_OK;
    const int rc = build_neighbours(w, dt);
    if (rc)
        report_reset(w);
    return rc;
} XPBD_ABI_CATCH

int xpbd_world_contacts_substep(xpbd_world *w, double h)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: NULL world");
    if (w->mode != XPBD_MODE_CONTACTS || (w->n && !w->have_neighbours))
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: call xpbd_world_contacts_begin first");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const int rc = substep_contacts(w, h, nullptr, 0);
    if (rc)
        report_reset(w);
    return rc;
} XPBD_ABI_CATCH

int xpbd_world_export_dynamic(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, double *dev_buf)
try {
    if (!w || (n && (!dev_indices || !dev_buf)))
        return set_error(XPBD_E_INVALID, "xpbd_world_export_dynamic: NULL argument");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_export_dynamic(w->arrays(), dev_indices, n, dev_buf, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_import_dynamic(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_buf)
try {
    if (!w || (n && (!dev_indices || !dev_buf)))
        return set_error(XPBD_E_INVALID, "xpbd_world_import_dynamic: NULL argument");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_import_dynamic(w->arrays(), dev_indices, nullptr, n, dev_buf, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_import_dynamic_rows(xpbd_world *w, const uint32_t *dev_indices, const uint32_t *dev_rows, uint32_t n,
                                   const double *dev_buf)
try {
    if (!w || (n && (!dev_indices || !dev_rows || !dev_buf)))
        return set_error(XPBD_E_INVALID, "xpbd_world_import_dynamic_rows: NULL argument");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_import_dynamic(w->arrays(), dev_indices, dev_rows, n, dev_buf, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_snapshot_positions(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, double *dev_snapshot)
try {
    if (!w || (n && (!dev_indices || !dev_snapshot)))
        return set_error(XPBD_E_INVALID, "xpbd_world_snapshot_positions: NULL argument");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_snapshot_positions(w->arrays(), dev_indices, n, dev_snapshot, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_max_displacement2(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_snapshot, const double *dev_scale,
                                 double *dev_max)
try {
    if (!w || !dev_max || (n && (!dev_indices || !dev_snapshot)))
        return set_error(XPBD_E_INVALID, "xpbd_world_max_displacement2: NULL argument");
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_max_displacement2(w->arrays(), dev_indices, n, dev_snapshot, dev_scale, dev_max, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_sat_schedule(xpbd_world *w, uint32_t schedule)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_sat_schedule: NULL world");
    if (schedule > XPBD_SAT_SCHEDULE_TWO_PASS)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_sat_schedule: unknown schedule %u", schedule);
    w->sat_schedule = schedule;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_narrowphase(xpbd_world *w, uint32_t narrowphase)
try {
    if (!w || (narrowphase != XPBD_NARROWPHASE_SAT && narrowphase != XPBD_NARROWPHASE_GJK_EPA))
        return set_error(XPBD_E_INVALID, "xpbd_world_set_narrowphase: bad argument");
    w->narrowphase = narrowphase;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_contact_pad(xpbd_world *w, double pad)
try {
    if (!w || !(pad >= 0.0) || pad > 1.0e6)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_pad: bad argument");
    w->contact_pad = pad;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_max_depenetration_speed(xpbd_world *w, double speed)
try {
    if (!w || !(speed >= 0.0) || speed > 1.0e300)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_max_depenetration_speed: bad argument");
    w->max_depenetration_speed = speed;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_contact_stats(xpbd_world *w, uint64_t out[3])
try {
    if (!w || !out)
        return set_error(XPBD_E_INVALID, "xpbd_world_contact_stats: NULL argument");
    out[0] = w->n_pairs;
    out[1] = out[2] = 0;
    if (!w->cb_stats.ptr)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    unsigned long long host[2] = {0, 0};
    XPBD_HIP_TRY(hipMemcpyAsync(host, w->cb_stats.ptr, 16, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->cb_stats.ptr, 0, 16, w->stream));
    w->stats_touching_seen = 0; // the schedule heuristic of build_neighbours starts counting afresh
    w->stats_pair_substeps_seen = w->stats_pair_substeps;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    out[1] = host[0];
    out[2] = host[1];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_contact_report(xpbd_world *w, uint32_t enable)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_report: NULL world");
    if (enable > 1u)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_report: enable must be 0 or 1, not %u", enable);
    if (int rc = bind_device(w))
        return rc;
    if (enable && !w->rep_host)
        XPBD_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->rep_host), 8 * sizeof(uint32_t), hipHostMallocDefault));
    if (!enable && w->report_on) { // (queued work may still read the buffers)
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
        for (DeviceBuffer *b : {&w->rep_touch, &w->rep_flag, &w->rep_sel, &w->rep_npts, &w->rep_keys[0], &w->rep_keys[1], &w->rep_scan,
                                &w->rep_ev_flag, &w->rep_pairs, &w->rep_points, &w->rep_events})
            b->release();
    }
    report_reset(w);
    w->report_on = enable != 0;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_contact_report_counts(xpbd_world *w, uint32_t out[4])
try {
    if (!w || !out)
        return set_error(XPBD_E_INVALID, "xpbd_world_contact_report_counts: NULL argument");
    XPBD_TRY(report_prepare(w, "xpbd_world_contact_report_counts"));
    for (int k = 0; k < 4; ++k)
        out[k] = w->report_counts[k];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_pair_contacts(xpbd_world *w, xpbd_pair_contact *pairs, uint32_t pair_cap, xpbd_contact_point *points,
                                      uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points)
try {
    if (!w || !n_pairs || !n_points || (!pairs && pair_cap) || (!points && point_cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_pair_contacts: NULL argument");
    XPBD_TRY(report_prepare(w, "xpbd_world_download_pair_contacts"));
    const uint32_t k = w->report_counts[0], total_points = w->report_counts[1];
    *n_pairs = k;
    *n_points = total_points;
    const uint32_t take = k < pair_cap ? k : pair_cap, take_points = points ? (total_points < point_cap ? total_points : point_cap) : 0u;
    if (take || take_points) {
        XPBD_HIP_TRY(w->rep_pairs.reserve((size_t)k * sizeof(xpbd_pair_contact)));
        if (points)
            XPBD_HIP_TRY(w->rep_points.reserve((size_t)(total_points ? total_points : 1) * sizeof(xpbd_contact_point)));
        const uint32_t cur = w->report_cur;
        XPBD_HIP_TRY(xpbd::launch_report_records(report_frame_of(w), w->rep_keys[cur].as<unsigned long long>(), w->rep_sel.as<uint32_t>(),
                                                 w->rep_npts.as<uint32_t>(), k, w->rep_pairs.as<xpbd_pair_contact>(),
                                                 points ? w->rep_points.as<xpbd_contact_point>() : nullptr, w->stream));
        if (take)
            XPBD_HIP_TRY(hipMemcpyAsync(pairs, w->rep_pairs.ptr, (size_t)take * sizeof(xpbd_pair_contact), hipMemcpyDeviceToHost, w->stream));
        if (take_points)
            XPBD_HIP_TRY(hipMemcpyAsync(points, w->rep_points.ptr, (size_t)take_points * sizeof(xpbd_contact_point), hipMemcpyDeviceToHost,
                                        w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (k > pair_cap || (points && total_points > point_cap))
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_pair_contacts: %u pairs, capacity %u; %u points, capacity %u", k, pair_cap,
                         total_points, point_cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_contact_events(xpbd_world *w, xpbd_contact_event *out, uint32_t cap, uint32_t *n_out)
try {
    if (!w || !n_out || (!out && cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_contact_events: NULL argument");
    XPBD_TRY(report_prepare(w, "xpbd_world_download_contact_events"));
    const uint32_t total = w->report_counts[2] + w->report_counts[3];
    *n_out = total;
    const uint32_t take = total < cap ? total : cap;
    if (take) {
        const uint32_t cur = w->report_cur, k = w->report_counts[0], n_prev = w->report_prev_valid ? w->rep_host[cur ^ 1u] : 0u;
        XPBD_HIP_TRY(w->rep_events.reserve((size_t)total * sizeof(xpbd_contact_event)));
        XPBD_HIP_TRY(xpbd::launch_report_event_write(w->rep_keys[cur].as<unsigned long long>(), k, w->rep_keys[cur ^ 1u].as<unsigned long long>(),
                                                     n_prev, w->rep_ev_flag.as<uint32_t>(), w->rep_events.as<xpbd_contact_event>(), w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(out, w->rep_events.ptr, (size_t)take * sizeof(xpbd_contact_event), hipMemcpyDeviceToHost, w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_contact_events: %u events, capacity %u", total, cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_build_neighbours(xpbd_world *w, double dt, uint32_t *n_entries_out)
try {
    if (!w || !n_entries_out)
        return set_error(XPBD_E_INVALID, "xpbd_world_build_neighbours: NULL argument");
    if (!w->has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_build_neighbours: call xpbd_world_set_polytopes first");
    if (int rc = bind_device(w))
        return rc;
    if (int rc = build_neighbours(w, dt))
        return rc;
    *n_entries_out = w->n_entries;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_neighbours(xpbd_world *w, uint32_t *offsets, uint32_t *neighbours, uint32_t cap)
try {
    if (!w || !offsets || (!neighbours && cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_neighbours: NULL argument");
    if (!w->have_neighbours)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_neighbours: no neighbour lists built yet");
    if (cap < w->n_entries)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_neighbours: %u entries, capacity %u", w->n_entries, cap);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(offsets, w->cb_nbr_off.ptr, (size_t)(w->n + 1) * 4, hipMemcpyDeviceToHost, w->stream));
    if (w->n_entries)
        XPBD_HIP_TRY(hipMemcpyAsync(neighbours, w->cb_nbr.ptr, (size_t)w->n_entries * 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_push(xpbd_world *w, uint32_t *index_out)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_push: NULL world");
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_push: no bodies uploaded");
    if (int rc = bind_device(w))
        return rc;
    const size_t slot = w->history_slot_bytes();
    if ((size_t)(w->history_length + 1) * slot > w->history.bytes) {
        // grow geometrically into a new block, carrying the old states over (device to device)
        uint32_t capacity = (uint32_t)(w->history.bytes / slot);
        capacity = capacity < 8 ? 8 : capacity * 2;
        DeviceBuffer bigger;
        hipError_t e = bigger.reserve((size_t)capacity * slot);
        if (e != hipSuccess)
            return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_world_history_push: %u states of %zu bytes: %s",
                             capacity, slot, hipGetErrorString(e));
        e = hipStreamSynchronize(w->stream);
        if (e == hipSuccess && w->history_length)
            e = hipMemcpy(bigger.ptr, w->history.ptr, (size_t)w->history_length * slot, hipMemcpyDeviceToDevice);
        if (e != hipSuccess)
            return set_error(XPBD_E_HIP, "xpbd_world_history_push: carrying %u states over failed: %s", w->history_length, hipGetErrorString(e));
        w->history = std::move(bigger); // (the old block goes with `bigger`)
    }
    char *dst = static_cast<char *>(w->history.ptr) + (size_t)w->history_length * slot;
    const size_t dyn_bytes = (size_t)xpbd::kDynFields * w->stride * 8;
    XPBD_HIP_TRY(hipMemcpyAsync(dst, w->dyn.ptr, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(dst + dyn_bytes, w->last_mask.ptr, (size_t)w->stride * 4, hipMemcpyDeviceToDevice, w->stream));
    w->history_stepped.push_back(w->stepped ? 1 : 0);
    if (index_out)
        *index_out = w->history_length;
    ++w->history_length;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_restore(xpbd_world *w, uint32_t index)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_restore: NULL world");
    if (index >= w->history_length)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_restore: state %u of %u", index, w->history_length);
    if (int rc = bind_device(w))
        return rc;
    const size_t slot = w->history_slot_bytes();
    const char *src = static_cast<const char *>(w->history.ptr) + (size_t)index * slot;
    const size_t dyn_bytes = (size_t)xpbd::kDynFields * w->stride * 8;
    XPBD_HIP_TRY(hipMemcpyAsync(w->dyn.ptr, src, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->last_mask.ptr, src + dyn_bytes, (size_t)w->stride * 4, hipMemcpyDeviceToDevice, w->stream));
    w->stepped = w->history_stepped[index] != 0;
    w->have_neighbours = false;
    report_reset(w);
    w->trace_rows = 0; // the per-substep trace belongs to the step call that was overwritten
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_history_truncate(xpbd_world *w, uint32_t length)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_truncate: NULL world");
    if (length > w->history_length)
        return set_error(XPBD_E_INVALID, "xpbd_world_history_truncate: length %u > %u", length, w->history_length);
    w->history_length = length;
    w->history_stepped.resize(length);
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_history_length(const xpbd_world *w) noexcept { return w ? w->history_length : 0; }

// ---- body edits (include/xpbd.h, "Body EDITS") ---------------------------------------------------------------------------------
namespace {
// Room in the staging buffers of the host variants (growing one frees the old block, which queued work may still use).
int reserve_edit_staging(xpbd_world *w, size_t index_bytes, size_t value_bytes, size_t list_bytes)
{
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->ed_indices, index_bytes}, {w->ed_values, value_bytes}, {w->ed_list, list_bytes}}));
    return XPBD_OK;
}

// The host variants' index list on the device (NULL: 0..n-1 written out, for the kernels that have no such form).
int stage_edit_indices(xpbd_world *w, const uint32_t *indices, uint32_t n, std::vector<uint32_t> &iota)
{
    if (!indices) {
        iota.resize(n);
        for (uint32_t k = 0; k < n; ++k)
            iota[k] = k;
        indices = iota.data();
    }
    XPBD_HIP_TRY(hipMemcpyAsync(w->ed_indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    return XPBD_OK;
}
} // namespace

int xpbd_world_set_external_wrench(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *force_xyz, const double *torque_xyz)
try {
    const char *who = "xpbd_world_set_external_wrench";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!force_xyz && !torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: force_xyz and torque_xyz are both NULL", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "force_xyz", force_xyz, (size_t)n * 3));
    XPBD_TRY(xpbd::check_edit_finite(who, "torque_xyz", torque_xyz, (size_t)n * 3));
    XPBD_TRY(bind_device(w));
    const size_t half = (size_t)n * 3 * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, 2 * half, 0));
    double *dev_force = w->ed_values.as<double>(), *dev_torque = dev_force + (size_t)n * 3;
    if (indices)
        XPBD_HIP_TRY(hipMemcpyAsync(w->ed_indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    if (force_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_force, force_xyz, half, hipMemcpyHostToDevice, w->stream));
    if (torque_xyz)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_torque, torque_xyz, half, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_set_wrench(w->arrays(), indices ? w->ed_indices.as<uint32_t>() : nullptr, n, force_xyz ? dev_force : nullptr,
                                         torque_xyz ? dev_torque : nullptr, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_external_wrench_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n, const double *dev_force_xyz,
                                          const double *dev_torque_xyz)
try {
    const char *who = "xpbd_world_set_external_wrench_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!dev_force_xyz && !dev_torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: dev_force_xyz and dev_torque_xyz are both NULL", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (!dev_indices && n != w->n)
        return set_error(XPBD_E_INVALID, "%s: dev_indices == NULL names the bodies 0..n-1, but n = %u and the world holds %u bodies", who, n, w->n);
    if (n > xpbd::kMaxEditEntries)
        return set_error(XPBD_E_INVALID, "%s: n = %u (at most %u entries per call)", who, n, xpbd::kMaxEditEntries);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_set_wrench(w->arrays(), dev_indices, n, dev_force_xyz, dev_torque_xyz, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_apply_impulses(xpbd_world *w, const xpbd_impulse *list, uint32_t n)
try {
    const char *who = "xpbd_world_apply_impulses";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(xpbd::check_impulses(who, list, n, w->n));
    // the device path wants the entries of a body adjacent; a stable sort keeps their order
    std::vector<xpbd_impulse> sorted(list, list + n);
    std::stable_sort(sorted.begin(), sorted.end(), [](const xpbd_impulse &a, const xpbd_impulse &b) { return a.body < b.body; });
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * sizeof(xpbd_impulse);
    XPBD_TRY(reserve_edit_staging(w, 0, 0, bytes));
    XPBD_HIP_TRY(hipMemcpyAsync(w->ed_list.ptr, sorted.data(), bytes, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_apply_impulses(w->arrays(), w->ed_list.as<xpbd_impulse>(), n, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // `sorted` is read by the copy
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_apply_impulses_device(xpbd_world *w, const xpbd_impulse *dev_list, uint32_t n)
try {
    const char *who = "xpbd_world_apply_impulses_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!dev_list)
        return set_error(XPBD_E_INVALID, "%s: NULL list", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    if (reinterpret_cast<uintptr_t>(dev_list) & 15u)
        return set_error(XPBD_E_INVALID, "%s: dev_list must be 16-byte aligned", who);
    if (n > xpbd::kMaxEditEntries)
        return set_error(XPBD_E_INVALID, "%s: n = %u (at most %u entries per call)", who, n, xpbd::kMaxEditEntries);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::launch_apply_impulses(w->arrays(), dev_list, n, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_set_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, const double *rows)
try {
    const char *who = "xpbd_world_set_dynamics";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "rows", rows, (size_t)n * xpbd::kDynFields));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kDynFields * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    std::vector<uint32_t> iota;
    XPBD_TRY(stage_edit_indices(w, indices, n, iota));
    XPBD_HIP_TRY(hipMemcpyAsync(w->ed_values.ptr, rows, bytes, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_import_dynamic(w->arrays(), w->ed_indices.as<uint32_t>(), nullptr, n, w->ed_values.as<double>(), w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_get_dynamics(xpbd_world *w, const uint32_t *indices, uint32_t n, double *rows)
try {
    const char *who = "xpbd_world_get_dynamics";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0)
        return XPBD_OK;
    if (!rows)
        return set_error(XPBD_E_INVALID, "%s: NULL rows", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, w->n, false));
    XPBD_TRY(bind_device(w));
    const size_t bytes = (size_t)n * xpbd::kDynFields * 8;
    XPBD_TRY(reserve_edit_staging(w, (size_t)n * 4, bytes, 0));
    std::vector<uint32_t> iota;
    XPBD_TRY(stage_edit_indices(w, indices, n, iota));
    XPBD_HIP_TRY(xpbd::launch_export_dynamic(w->arrays(), w->ed_indices.as<uint32_t>(), n, w->ed_values.as<double>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(rows, w->ed_values.ptr, bytes, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

// ---- body population (include/xpbd.h, "Body POPULATION") -----------------------------------------------------------------------
namespace {
// Everything a population change replaces, built aside: the body arrays at the new stride, the per-body tables that are on, the
// scratch sized by the stride, and the joint tables.  Only commit_population touches the world, after every allocation, copy
// and launch has succeeded; a stage that is dropped frees its blocks and leaves the previous population in force.
struct PopulationStage {
    uint32_t n = 0, stride = 0;
    DeviceBuffer dyn, stat, shape_id, last_mask, aos_staging, filters, friction, restitution, dyn_alt, rs_start;
    JointTables joints;
};

// The new body arrays and per-body tables: new body s < n_keep is the present body dev_src[s] (NULL: body s), the n_add bodies
// of `aos` follow.  Device bound, stream idle; enqueues on the world's stream and does not wait.
int stage_bodies(xpbd_world *w, const uint32_t *dev_src, uint32_t n_keep, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n_add,
                 PopulationStage &st)
{
    // (adopt_body_count's bound, before the sum can wrap: this is the other way a world comes by its body count)
    if (n_keep > kMaxBodies || n_add > kMaxBodies - n_keep)
        return set_error(XPBD_E_INVALID, "a world holds at most %u bodies, not %u + %u", kMaxBodies, n_keep, n_add);
    const uint32_t n_new = n_keep + n_add, stride = stride_for(n_new);
    st.n = n_new;
    st.stride = stride;
    XPBD_HIP_TRY(st.dyn.reserve((size_t)xpbd::kDynFields * stride * 8));
    XPBD_HIP_TRY(st.stat.reserve((size_t)xpbd::kStatFields * stride * 8));
    XPBD_HIP_TRY(st.shape_id.reserve((size_t)stride * 4));
    XPBD_HIP_TRY(st.last_mask.reserve((size_t)stride * 4));
    const size_t aos_bytes = (size_t)(n_new ? n_new : 1) * sizeof(xpbd_rigid);
    if (w->aos_staging.bytes < aos_bytes) // (xpbd_world_download_bodies stages n bodies there)
        XPBD_HIP_TRY(st.aos_staging.reserve(aos_bytes));
    XPBD_HIP_TRY(hipMemsetAsync(st.last_mask.ptr, 0, (size_t)stride * 4, w->stream));
    const xpbd::BodyArrays fresh{st.dyn.as<double>(), st.stat.as<double>(), st.shape_id.as<uint32_t>(), stride, n_new};
    XPBD_HIP_TRY(xpbd::launch_population_gather_bodies(w->arrays(), fresh, dev_src, n_keep, w->stream));
    if (n_add) {
        // the appended bodies take k_aos_to_soa's tile path into the same arrays, from slot n_keep on
        double *incoming = (st.aos_staging.ptr ? st.aos_staging : w->aos_staging).as<double>();
        XPBD_HIP_TRY(hipMemcpyAsync(incoming, aos, (size_t)n_add * sizeof(xpbd_rigid), hipMemcpyHostToDevice, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(fresh.shape_id + n_keep, shape_id, (size_t)n_add * 4, hipMemcpyHostToDevice, w->stream));
        const xpbd::BodyArrays tail{fresh.dyn + n_keep, fresh.stat + n_keep, fresh.shape_id + n_keep, stride, n_add};
        XPBD_HIP_TRY(xpbd::launch_aos_to_soa(incoming, tail, w->stream));
    }
    // the per-body tables: a table that is off stays off; an appended body gets the default
    if (w->filters.on) {
        XPBD_HIP_TRY(st.filters.reserve((size_t)(n_new ? n_new : 1) * sizeof(uint2)));
        XPBD_HIP_TRY(xpbd::launch_population_gather_filters(w->ft_filters.as<uint2>(), st.filters.as<uint2>(), dev_src, n_keep, n_new,
                                                            uint2{~0u, ~0u}, w->stream));
    }
    if (w->materials.on) {
        XPBD_HIP_TRY(st.friction.reserve((size_t)(n_new ? n_new : 1) * 8));
        XPBD_HIP_TRY(xpbd::launch_population_gather_doubles(w->mt_friction.as<double>(), st.friction.as<double>(), dev_src, n_keep, n_new,
                                                            std::numeric_limits<double>::infinity(), w->stream));
    }
    if (w->restitution.on) {
        XPBD_HIP_TRY(st.restitution.reserve((size_t)(n_new ? n_new : 1) * 8));
        XPBD_HIP_TRY(xpbd::launch_population_gather_doubles(w->rs_restitution.as<double>(), st.restitution.as<double>(), dev_src, n_keep, n_new, 0.0,
                                                            w->stream));
        if (w->dyn_alt.bytes < (size_t)xpbd::kDynFields * stride * 8) // the velocity pass's scratch follows the stride
            XPBD_HIP_TRY(st.dyn_alt.reserve((size_t)xpbd::kDynFields * stride * 8));
        if (w->rs_start.bytes < (size_t)6 * stride * 8)
            XPBD_HIP_TRY(st.rs_start.reserve((size_t)6 * stride * 8));
    }
    return XPBD_OK;
}

// Nothing here can fail.  The old blocks leave with the stage.
void commit_population(xpbd_world *w, PopulationStage &st, uint32_t max_shape_id)
{
    auto take = [](DeviceBuffer &mine, DeviceBuffer &fresh) {
        if (fresh.ptr)
            mine = std::move(fresh);
    };
    take(w->dyn, st.dyn);
    take(w->stat, st.stat);
    take(w->shape_id, st.shape_id);
    take(w->last_mask, st.last_mask);
    take(w->aos_staging, st.aos_staging);
    take(w->ft_filters, st.filters);
    take(w->mt_friction, st.friction);
    take(w->rs_restitution, st.restitution);
    take(w->dyn_alt, st.dyn_alt);
    take(w->rs_start, st.rs_start);
    w->joints = std::move(st.joints);
    take_body_count(w, st.n, max_shape_id);
}

// Both variants of xpbd_world_remove_bodies, after their checks: the removal flags are on the device (dev_remove), or
// `indices` still has to be scattered into the world's own flag array (dev_remove == NULL).
int remove_bodies(xpbd_world *w, const uint8_t *dev_remove, const uint32_t *indices, uint32_t n_indices, uint32_t *old_to_new,
                  uint32_t *dev_old_to_new, uint32_t *joint_old_to_new, uint32_t *n_bodies_out)
{
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the scratch below may move, and the old arrays are freed at the end
    const uint32_t n = w->n;
    XPBD_HIP_TRY(w->pop_prefix.reserve(((size_t)n + 1) * 4));
    XPBD_HIP_TRY(w->pop_scan.reserve(((size_t)n / 1024 + 8) * 4));
    XPBD_HIP_TRY(w->pop_map.reserve((size_t)n * 4));
    XPBD_HIP_TRY(w->pop_src.reserve((size_t)n * 4));
    if (!dev_remove) {
        XPBD_HIP_TRY(w->pop_remove.reserve(n));
        XPBD_HIP_TRY(w->pop_indices.reserve((size_t)n_indices * 4));
        XPBD_HIP_TRY(hipMemsetAsync(w->pop_remove.ptr, 0, n, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(w->pop_indices.ptr, indices, (size_t)n_indices * 4, hipMemcpyHostToDevice, w->stream));
        XPBD_HIP_TRY(xpbd::launch_population_mark(w->pop_indices.as<uint32_t>(), n_indices, w->pop_remove.as<uint8_t>(), n, w->stream));
        dev_remove = w->pop_remove.as<uint8_t>();
    }
    XPBD_HIP_TRY(xpbd::launch_population_map(dev_remove, n, w->pop_prefix.as<uint32_t>(), w->pop_scan.as<uint32_t>(), w->pop_map.as<uint32_t>(),
                                             w->pop_src.as<uint32_t>(), w->stream));
    uint32_t n_keep = 0;
    XPBD_HIP_TRY(hipMemcpyAsync(&n_keep, w->pop_prefix.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, w->stream));
    std::vector<uint32_t> map; // on the host only for the caller or for the joint re-index
    if (old_to_new || w->joints.csr.n) {
        map.resize(n);
        XPBD_HIP_TRY(hipMemcpyAsync(map.data(), w->pop_map.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, w->stream));
    }
    if (dev_old_to_new)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_old_to_new, w->pop_map.ptr, (size_t)n * 4, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    if (n_keep > n)
        return set_error(XPBD_E_HIP, "xpbd_world_remove_bodies: the scan left %u survivors of %u bodies", n_keep, n);
    std::vector<uint32_t> joint_map(w->joints.csr.n);
    if (n_keep == n) { // (the device variant with no flag set) nobody leaves: nothing changes, history and the rest stay
        for (uint32_t j = 0; j < w->joints.csr.n; ++j)
            joint_map[j] = j;
    } else {
        PopulationStage st;
        if (w->joints.csr.n)
            XPBD_TRY(stage_joint_tables(xpbd::remap_joint_set(w->joints.set, map.data(), n, joint_map), n_keep, w->stream, st.joints));
        XPBD_TRY(stage_bodies(w, w->pop_src.as<uint32_t>(), n_keep, nullptr, nullptr, 0, st));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
        commit_population(w, st, w->max_shape_id); // (max_shape_id stays an upper bound)
        if (n_keep == 0)
            w->stat_shared = false; // as after an upload of no bodies
    }
    if (old_to_new)
        std::memcpy(old_to_new, map.data(), (size_t)n * 4);
    if (joint_old_to_new && !joint_map.empty())
        std::memcpy(joint_old_to_new, joint_map.data(), joint_map.size() * 4);
    if (n_bodies_out)
        *n_bodies_out = n_keep;
    return XPBD_OK;
}
} // namespace

int xpbd_world_remove_bodies(xpbd_world *w, const uint32_t *indices, uint32_t n, uint32_t *old_to_new, uint32_t *joint_old_to_new,
                             uint32_t *n_bodies_out)
try {
    const char *who = "xpbd_world_remove_bodies";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n == 0) { // nothing at all: the maps are the identity
        for (uint32_t i = 0; old_to_new && i < w->n; ++i)
            old_to_new[i] = i;
        for (uint32_t j = 0; joint_old_to_new && j < w->joints.csr.n; ++j)
            joint_old_to_new[j] = j;
        if (n_bodies_out)
            *n_bodies_out = w->n;
        return XPBD_OK;
    }
    if (!indices)
        return set_error(XPBD_E_INVALID, "%s: NULL indices with n = %u", who, n);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    for (uint32_t k = 0; k < n; ++k)
        if (indices[k] >= w->n)
            return set_error(XPBD_E_INVALID, "%s: indices[%u] = %u but the world holds %u bodies", who, k, indices[k], w->n);
    return remove_bodies(w, nullptr, indices, n, old_to_new, nullptr, joint_old_to_new, n_bodies_out);
} XPBD_ABI_CATCH

int xpbd_world_remove_bodies_device(xpbd_world *w, const uint8_t *dev_remove, uint32_t *dev_old_to_new, uint32_t *joint_old_to_new,
                                    uint32_t *n_bodies_out)
try {
    const char *who = "xpbd_world_remove_bodies_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (!dev_remove)
        return set_error(XPBD_E_INVALID, "%s: NULL dev_remove", who);
    if (w->n == 0)
        return set_error(XPBD_E_INVALID, "%s: the world holds no bodies", who);
    return remove_bodies(w, dev_remove, nullptr, 0, nullptr, dev_old_to_new, joint_old_to_new, n_bodies_out);
} XPBD_ABI_CATCH

int xpbd_world_add_bodies(xpbd_world *w, const xpbd_rigid *aos, const uint32_t *shape_id, uint32_t n_add, uint32_t *first_index_out)
try {
    const char *who = "xpbd_world_add_bodies";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (n_add == 0) {
        if (first_index_out)
            *first_index_out = w->n;
        return XPBD_OK;
    }
    if (!aos || !shape_id)
        return set_error(XPBD_E_INVALID, "%s: NULL aos or shape_id with n_add = %u", who, n_add);
    if (w->n_shapes == 0)
        return set_error(XPBD_E_INVALID, "%s: call xpbd_world_set_shapes first", who);
    if (n_add > std::numeric_limits<uint32_t>::max() - 256u - w->n) // (the stride rounds the count up to a multiple of 256)
        return set_error(XPBD_E_INVALID, "%s: %u + %u bodies exceed what xpbd_world_upload_bodies accepts", who, w->n, n_add);
    uint32_t max_shape_id = w->n ? w->max_shape_id : 0u;
    for (uint32_t i = 0; i < n_add; ++i) {
        if (shape_id[i] >= w->n_shapes)
            return set_error(XPBD_E_INVALID, "%s: shape_id[%u] = %u >= n_shapes %u", who, i, shape_id[i], w->n_shapes);
        max_shape_id = shape_id[i] > max_shape_id ? shape_id[i] : max_shape_id;
    }
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the old arrays are freed at the end
    const uint32_t first = w->n;
    PopulationStage st;
    if (w->joints.csr.n) // the same joints in a world of more bodies: the CSR body -> joints grows
        XPBD_TRY(stage_joint_tables(w->joints.set, first + n_add, w->stream, st.joints));
    XPBD_TRY(stage_bodies(w, nullptr, first, aos, shape_id, n_add, st));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's arrays are only borrowed
    commit_population(w, st, max_shape_id);
    // mass properties shared per shape: the bodies that stay kept the property, the appended ones are checked (a world that
    // was empty starts over, as an upload does)
    reset_stat_records(w, first == 0, n_add);
    for (uint32_t i = 0; i < n_add && w->stat_shared; ++i)
        absorb_stat_record(w, aos[i], shape_id[i]);
    if (first_index_out)
        *first_index_out = first;
    return XPBD_OK;
} XPBD_ABI_CATCH

namespace {
// The scene queries' argument checks (xpbd::check_raycast, xpbd::check_overlap, xpbd::check_sweep) against one world.
xpbd::QueryTarget query_target(const xpbd_world *w)
{
    return {w->has_topology, w->n, w->n_shapes, "xpbd_world_set_polytopes (set_shapes gives vertices only)", true, w->terrain.planes != nullptr};
}

int check_world_raycast(const char *who, const xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, const void *hits, bool host)
{
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    return xpbd::check_raycast(who, query_target(w), rays, n_rays, flags, hits, host);
}

int check_world_overlap(const char *who, const xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags,
                        const void *offsets, const void *hits, uint32_t cap, const uint32_t *n_out, bool host)
{
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    return xpbd::check_overlap(who, query_target(w), queries, n_queries, flags, offsets, hits, cap, n_out, host);
}
} // namespace

int xpbd_world_raycast(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits)
try {
    if (int rc = check_world_raycast("xpbd_world_raycast", w, rays, n_rays, flags, hits, true))
        return rc;
    return xpbd::raycast_host(w, rays, n_rays, flags, hits, nullptr, false, 0u);
} XPBD_ABI_CATCH

int xpbd_world_raycast_masked(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, uint32_t mask, xpbd_ray_hit *hits)
try {
    if (int rc = check_world_raycast("xpbd_world_raycast_masked", w, rays, n_rays, flags, hits, true))
        return rc;
    return xpbd::raycast_host(w, rays, n_rays, flags, hits, nullptr, true, mask);
} XPBD_ABI_CATCH

int xpbd_world_raycast_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *dev_hits)
try {
    if (int rc = check_world_raycast("xpbd_world_raycast_device", w, dev_rays, n_rays, flags, dev_hits, false))
        return rc;
    return xpbd::raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, nullptr, false, 0u);
} XPBD_ABI_CATCH

int xpbd_world_raycast_masked_device(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, uint32_t mask,
                                     xpbd_ray_hit *dev_hits)
try {
    if (int rc = check_world_raycast("xpbd_world_raycast_masked_device", w, dev_rays, n_rays, flags, dev_hits, false))
        return rc;
    return xpbd::raycast_enqueue(w, dev_rays, n_rays, flags, dev_hits, nullptr, true, mask);
} XPBD_ABI_CATCH

int xpbd_world_overlap(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                       xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
try {
    if (int rc = check_world_overlap("xpbd_world_overlap", w, queries, n_queries, flags, offsets, hits, cap, n_out, true))
        return rc;
    uint32_t total = 0;
    const int rc = xpbd::overlap_host(w, queries, n_queries, flags, offsets, hits, cap, &total, nullptr);
    if (n_out && (rc == XPBD_OK || rc == XPBD_E_CAPACITY))
        *n_out = total;
    return rc;
} XPBD_ABI_CATCH

int xpbd_world_overlap_device(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags, uint32_t *dev_offsets,
                              xpbd_overlap_hit *dev_hits, uint32_t cap)
try {
    if (int rc = check_world_overlap("xpbd_world_overlap_device", w, dev_queries, n_queries, flags, dev_offsets, dev_hits, cap, nullptr, false))
        return rc;
    return xpbd::overlap_enqueue(w, dev_queries, n_queries, flags, dev_offsets, dev_hits, cap, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_sweep(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_sweep: NULL world");
    if (int rc = xpbd::check_sweep("xpbd_world_sweep", query_target(w), sweeps, n_sweeps, flags, hits, true))
        return rc;
    return xpbd::sweep_host(w, sweeps, n_sweeps, flags, hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_world_sweep_device(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *dev_hits)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_sweep_device: NULL world");
    if (int rc = xpbd::check_sweep("xpbd_world_sweep_device", query_target(w), dev_sweeps, n_sweeps, flags, dev_hits, false))
        return rc;
    return xpbd::sweep_enqueue(w, dev_sweeps, n_sweeps, flags, dev_hits, nullptr);
} XPBD_ABI_CATCH

int xpbd_selftest_div_sqrt(int32_t device, const double *a, const double *b, double *quotient, double *root,
                           uint32_t n)
try {
    if (n && (!a || !b || !quotient || !root))
        return set_error(XPBD_E_INVALID, "xpbd_selftest_div_sqrt: NULL argument");
    if (n == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipSetDevice(device));
    DeviceBuffer buf;
    const size_t bytes = (size_t)n * 8;
    hipError_t e = buf.reserve(4 * bytes);
    if (e != hipSuccess)
        return set_error(XPBD_E_OOM, "xpbd_selftest_div_sqrt: %s", hipGetErrorString(e));
    double *d = buf.as<double>();
    e = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = xpbd::launch_selftest_div_sqrt(d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(quotient, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(root, d + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return set_error(XPBD_E_HIP, "xpbd_selftest_div_sqrt: %s", hipGetErrorString(e));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_hbm_copy(int32_t device, uint64_t bytes, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || bytes < 16 || bytes >= (1ull << 40) || repeats == 0)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_hbm_copy: bad argument");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    bytes &= ~(uint64_t)15;
    DeviceBuffer src, dst;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = src.reserve(bytes);
    if (e == hipSuccess) e = dst.reserve(bytes);
    if (e == hipSuccess) e = hipMemset(src.ptr, 0x3c, bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t variant = 0; variant < xpbd::kCopyVariants && e == hipSuccess; ++variant) { // report the fastest kernel
        const uint32_t nt = variant;
        e = xpbd::launch_copy16(src.ptr, dst.ptr, bytes, nt, nullptr); // warm-up (page tables, clocks)
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        for (uint32_t k = 0; k < repeats && e == hipSuccess; ++k)
            e = xpbd::launch_copy16(src.ptr, dst.ptr, bytes, nt, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && (variant == 0 || ms < best_ms))
            best_ms = ms;
    }
    const float ms = best_ms;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_hbm_copy: %s", hipGetErrorString(e));
    *gbytes_per_s = 2.0 * (double)bytes * repeats / ((double)ms * 1e-3) / 1e9; // bytes read + bytes written
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_gather(int32_t device, uint32_t records, uint32_t record_bytes, uint32_t read_bytes, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || records < 256 || (records & (records - 1)) != 0 || repeats == 0 || read_bytes > record_bytes)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_gather: records must be a power of two >= 256, read_bytes <= record_bytes");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    const size_t in_bytes = (size_t)records * record_bytes, out_bytes = (size_t)records * 8;
    DeviceBuffer in, out;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = in.reserve(in_bytes);
    if (e == hipSuccess) e = out.reserve(out_bytes);
    if (e == hipSuccess) e = hipMemset(in.ptr, 0, in_bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t k = 0; k < repeats + 1 && e == hipSuccess; ++k) { // (the first launch warms up and is not counted)
        e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = xpbd::launch_gather_records(in.ptr, out.as<double>(), records, record_bytes, read_bytes, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && k > 0 && (k == 1 || ms < best_ms))
            best_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e == hipErrorInvalidValue)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_gather: no kernel for %u bytes read of %u-byte records", read_bytes, record_bytes);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_gather: %s", hipGetErrorString(e));
    *gbytes_per_s = ((double)records * read_bytes + (double)out_bytes) / ((double)best_ms * 1e-3) / 1e9;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_field_streams(int32_t device, uint64_t bodies, uint32_t tile_major, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || bodies < 64 || bodies > (1ull << 28) || repeats == 0)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_field_streams: bad argument");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    bodies = (bodies + 63) / 64 * 64;
    const size_t in_bytes = (size_t)bodies * (xpbd::kDynFields + xpbd::kStatFields) * 8, out_bytes = (size_t)bodies * xpbd::kDynFields * 8;
    DeviceBuffer in, out;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = in.reserve(in_bytes);
    if (e == hipSuccess) e = out.reserve(out_bytes);
    if (e == hipSuccess) e = hipMemset(in.ptr, 0, in_bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t k = 0; k < repeats + 1 && e == hipSuccess; ++k) { // (the first launch warms up and is not counted)
        e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = xpbd::launch_field_streams(in.as<double>(), out.as<double>(), bodies, tile_major != 0, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && k > 0 && (k == 1 || ms < best_ms))
            best_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_field_streams: %s", hipGetErrorString(e));
    *gbytes_per_s = (double)(in_bytes + out_bytes) / ((double)best_ms * 1e-3) / 1e9;
    return XPBD_OK;
} XPBD_ABI_CATCH

} // extern "C"

namespace xpbd {
int report_shard(xpbd_world *w, const uint8_t *dev_owned, const uint32_t *dev_global_id, std::vector<xpbd_pair_contact> &pairs,
                 std::vector<xpbd_contact_point> &points) noexcept
try {
    pairs.clear();
    points.clear();
    if (!w)
        return set_error(XPBD_E_INVALID, "report_shard: NULL world");
    if (w->n == 0)
        return XPBD_OK;
    // the keys are compacted again with the shard's mapping, and once more without it should the shard world itself be asked
    w->rep_map_owned = dev_owned;
    w->rep_map_ids = dev_global_id;
    w->report_keys_ready = w->report_ready = false;
    uint32_t counts[4] = {0, 0, 0, 0}, n_pairs = 0, n_points = 0;
    int rc = xpbd_world_contact_report_counts(w, counts);
    if (rc == XPBD_OK) {
        pairs.resize(counts[0]);
        points.resize(counts[1]);
        rc = xpbd_world_download_pair_contacts(w, pairs.empty() ? nullptr : pairs.data(), counts[0], points.empty() ? nullptr : points.data(),
                                               counts[1], &n_pairs, &n_points);
    }
    w->rep_map_owned = nullptr;
    w->rep_map_ids = nullptr;
    w->report_keys_ready = w->report_ready = false;
    return rc;
} catch (...) {
    w->rep_map_owned = nullptr;
    w->rep_map_ids = nullptr;
    w->report_keys_ready = w->report_ready = false;
    return abi_exception("report_shard");
}
} // namespace xpbd
