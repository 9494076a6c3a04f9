// xpbd_world_contacts.cpp -- the contact pipeline of the single-GPU world (XPBD_MODE_CONTACTS): both halves of the broadphase,
// the narrowphase schedule, the fused and the unfused substeps, the pieces of a shard's frame split at the halo exchange, and
// the entry points of the split API.
#include "xpbd_world.hpp"
#include "xpbd_body_ops.h"
#include "xpbd_scan.h"

void NarrowphaseSchedule::choose(unsigned long long touching_now, uint32_t two_classes)
{
    // Pre-test as a pass of its own for the coming frame?  Either way the results are the same bits; this only
    // picks the cheaper schedule from how many of the pairs examined since the last broadphase were touching.
    // SAT: the pre-test pass also answers the pairs whose cached face axis still separates them (SatScratch), so it
    // pays unless nearly every pair touches (box stacks: 99 % touching, one pass 5 % faster; a pile of boxes with
    // 40 % touching: two passes 35 % faster).  (GJK + EPA always runs the pre-test as a pass of its own: see
    // narrowphase_contacts.)
    const unsigned long long touching = touching_now - stats_touching_seen;
    const unsigned long long examined = stats_pair_substeps - stats_pair_substeps_seen;
    if (sat_schedule != XPBD_SAT_SCHEDULE_AUTO)
        sat_two_pass = sat_schedule == XPBD_SAT_SCHEDULE_TWO_PASS;
    else if (examined)
        sat_two_pass = touching * 5 < examined * 4;
    if (sat_schedule == XPBD_SAT_SCHEDULE_AUTO && two_classes)
        sat_two_pass = true; // small and large shapes: the two-pass form sorts the pairs by class (xpbd_pairs.h)
    // A DENSE scene (>= 15 % of the pairs examined in the last frame touched)?  Then (a) separating EDGE axes go into the
    // axis cache (SatScratch): trying one costs the pre-test a whole edge query for every wave that holds such a pair; it
    // pays where many pairs are close (piles: 35-40 % of the pairs touch, +4 % / +9 %), not where a few are (chains of
    // spaced boxes: 5 % touch, -4 %); and (b) box pairs run in groups of four lanes instead of eight (for_shape_maxima:
    // piles and stacks +7 %, the chains -3 %).  Same bits either way.
    if (examined)
        sat_scratch.cache_edge_axes = touching * 100 >= examined * 15;
    stats_touching_seen = touching_now;
    stats_pair_substeps_seen = stats_pair_substeps;
}

int NarrowphaseSchedule::ensure_gjk_scratch(uint32_t n_pairs, hipStream_t stream)
{
    if (!gjk_counters.ptr) {
        XPBD_HIP_TRY(gjk_counters.reserve(xpbd::gjk_counter_bytes()));
        XPBD_HIP_TRY(hipMemsetAsync(gjk_counters.ptr, 0, xpbd::gjk_counter_bytes(), stream));
        gjk_scratch.calls = 0;
    }
    XPBD_HIP_TRY(gjk_pairs_scratch.reserve(xpbd::gjk_scratch_bytes(at_least_one(n_pairs))));
    gjk_scratch.counters = gjk_counters.as<uint32_t>();
    gjk_scratch.pairs_scratch = gjk_pairs_scratch.ptr;
    return XPBD_OK;
}

// Sphere broadphase of the contact pipeline: neighbour lists + pair list for the coming frame, in two halves.
// First half: bounding spheres, buckets and the neighbour COUNT of every body are enqueued, the totals travel to pinned host
// memory behind them, an event marks their arrival.  Nothing here waits for the device.
int build_neighbours_enqueue(xpbd_world *w, double dt)
{
    if (int rc = w->report.frame_end(w))
        return rc;
    if (w->sleep.on) // the wake requests made since the last frame, and who is inert in this one
        XPBD_TRY(w->sleep.frame_begin(w));
    if (!w->bp.totals) {
        XPBD_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->bp.totals), sizeof *w->bp.totals, hipHostMallocDefault));
        XPBD_HIP_TRY(hipEventCreateWithFlags(&w->bp.event, hipEventDisableTiming));
    }
    const uint32_t n = w->n, st = w->stride;
    w->bp.table_size = next_pow2(n < 512 ? 1024 : 2 * n);
    XPBD_HIP_TRY(w->bp.centers.reserve((size_t)3 * st * 8));
    XPBD_HIP_TRY(w->bp.radius.reserve((size_t)st * 8));
    XPBD_HIP_TRY(w->bp.cell.reserve((size_t)3 * st * 4));
    XPBD_HIP_TRY(w->bp.key.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->bp.maxr.reserve(sizeof(xpbd::GridInfo)));
    XPBD_HIP_TRY(w->bp.grid_partials.reserve(((size_t)st / 256 + 1) * 7 * 8));
    XPBD_HIP_TRY(w->bp.bucket_start.reserve((size_t)(w->bp.table_size + 1) * 4));
    XPBD_HIP_TRY(w->bp.bucket_cursor.reserve((size_t)w->bp.table_size * 4));
    XPBD_HIP_TRY(w->bp.items.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->bp.items_unsorted.reserve((size_t)st * 4));
    XPBD_HIP_TRY(w->bp.slot_sphere.reserve((size_t)4 * st * 8));
    XPBD_HIP_TRY(w->bp.slot_cell.reserve((size_t)3 * st * 4));
    if (w->filters.on)
        XPBD_HIP_TRY(w->bp.slot_filter.reserve((size_t)2 * st * 4));
    if (w->sleep.on)
        XPBD_HIP_TRY(w->bp.slot_inert.reserve((size_t)st));
    XPBD_HIP_TRY(w->bp.nbr_off.reserve((size_t)(st + 1) * 4));
    XPBD_HIP_TRY(w->bp.pair_first.reserve((size_t)(st + 1) * 4));
    XPBD_HIP_TRY(w->bp.upper_start.reserve((size_t)st * 4));
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
    XPBD_HIP_TRY(w->bp.scan.reserve(xpbd::scan_scratch_bytes(w->bp.table_size > st ? w->bp.table_size : st)));
    if (!w->np.stats.ptr) {
        XPBD_HIP_TRY(w->np.stats.reserve(16));
        XPBD_HIP_TRY(hipMemsetAsync(w->np.stats.ptr, 0, 16, w->stream));
        w->np.stats_touching_seen = 0;
        w->np.stats_pair_substeps_seen = w->np.stats_pair_substeps;
    }
    const xpbd::BodyArrays b = w->arrays();
    xpbd::ContactBuffers c = w->contact_buffers();
    XPBD_HIP_TRY(xpbd::launch_bounds_and_cells(b, w->geom.tables(), w->geom.radii.as<double>(), dt, w->contact_pad, c,
                                               w->stream));
    XPBD_HIP_TRY(xpbd::launch_build_buckets(b, c, w->stream, w->inert_bodies()));
    XPBD_HIP_TRY(xpbd::launch_neighbour_count(b, c, w->stream, w->inert_bodies()));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->bp.totals->entries, c.nbr_off + n, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&w->bp.totals->pairs, c.pair_first + n, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->bp.totals->stats, c.stats, 16, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipEventRecord(w->bp.event, w->stream));
    w->bp.pending = true;
    w->bp.have_neighbours = false;
    return XPBD_OK;
}

// Second half: waits for the totals (the one host synchronisation of a frame in XPBD_MODE_CONTACTS), sizes the pair
// buffers and fills the neighbour and pair lists.
int build_neighbours_collect(xpbd_world *w)
{
    if (!w->bp.pending)
        return set_error(XPBD_E_INVALID, "build_neighbours_collect without build_neighbours_enqueue");
    XPBD_HIP_TRY(hipEventSynchronize(w->bp.event));
    w->bp.pending = false;
    const xpbd::BodyArrays b = w->arrays();
    xpbd::ContactBuffers c = w->contact_buffers();
    w->bp.n_entries = w->bp.totals->entries;
    w->bp.n_pairs = w->bp.totals->pairs;
    w->np.choose(w->bp.totals->stats[0], w->geom.two_classes);
    if (!w->np.sat_counters.ptr) {
        XPBD_HIP_TRY(w->np.sat_counters.reserve(2 * xpbd::kSurvivorCounters * 4));
        XPBD_HIP_TRY(hipMemsetAsync(w->np.sat_counters.ptr, 0, 2 * xpbd::kSurvivorCounters * 4, w->stream));
        w->np.sat_scratch.calls = 0;
    }
    XPBD_HIP_TRY(w->np.sat_survivors.reserve((size_t)at_least_one(w->bp.n_pairs) * 2 * 4)); // 2 * n_pairs entries: SatScratch
    // the pair list is new: nothing is known about which axis separates which pair
    XPBD_HIP_TRY(w->np.sat_axis_cache.reserve((size_t)at_least_one(w->bp.n_pairs) * 2));
    XPBD_HIP_TRY(hipMemsetAsync(w->np.sat_axis_cache.ptr, 0, (size_t)at_least_one(w->bp.n_pairs) * 2, w->stream));
    w->np.sat_scratch.counters = w->np.sat_counters.as<uint32_t>();
    w->np.sat_scratch.survivors = w->np.sat_survivors.as<uint32_t>();
    w->np.sat_scratch.axis_cache = w->np.sat_axis_cache.as<uint16_t>();
    if (w->narrowphase == XPBD_NARROWPHASE_GJK_EPA) {
        XPBD_HIP_TRY(w->np.gjk_axis_cache.reserve((size_t)at_least_one(w->bp.n_pairs) * 24));
        XPBD_HIP_TRY(hipMemsetAsync(w->np.gjk_axis_cache.ptr, 0, (size_t)at_least_one(w->bp.n_pairs) * 24, w->stream));
    }
    XPBD_HIP_TRY(w->bp.nbr.reserve((size_t)at_least_one(w->bp.n_entries) * 4));
    XPBD_HIP_TRY(w->bp.nbr_pair.reserve((size_t)at_least_one(w->bp.n_entries) * 4));
    XPBD_HIP_TRY(w->bp.pairs.reserve((size_t)at_least_one(w->bp.n_pairs) * 8));
    XPBD_HIP_TRY(w->bp.manifolds.reserve((size_t)at_least_one(w->bp.n_pairs) * sizeof(xpbd::ContactManifold)));
    XPBD_HIP_TRY(w->bp.pair_codes.reserve((size_t)at_least_one(w->bp.n_pairs)));
    c = w->contact_buffers();
    XPBD_HIP_TRY(xpbd::launch_neighbour_fill(b, c, w->stream, w->inert_bodies()));
    w->bp.have_neighbours = true;
    return w->report.frame_begin(w);
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
        if (int rc = w->np.ensure_gjk_scratch(w->bp.n_pairs, w->stream))
            return rc;
        // always with the pre-test as a pass of its own: that pass consults the cached separating directions, which are
        // part of the narrowphase's semantics (og_gjk_epa_cached of the oracle), not a schedule
        w->np.gjk_scratch.axis_cache = w->np.gjk_axis_cache.as<double>();
        w->np.gjk_scratch.codes = c.pair_codes;
        XPBD_HIP_TRY(xpbd::launch_gjk_epa_pairs(b, w->geom.tables(), c.rec, c.pairs, w->bp.n_pairs, nullptr, c.manifolds,
                                                w->np.gjk_scratch, true, &w->np.sat_scratch, w->stream));
    } else {
        XPBD_HIP_TRY(xpbd::launch_sat_contact_pairs(b, w->geom.tables(), c, w->bp.n_pairs, w->np.sat_two_pass ? &w->np.sat_scratch : nullptr,
                                                    w->stream, w->np.sat_scratch.cache_edge_axes /* = a dense scene, see below */));
    }
    w->np.stats_pair_substeps += w->bp.n_pairs;
    if (int rc = w->report.note_substep(w, c.pair_codes))
        return rc;
    return sensor_mask_codes(w, c); // what solve_buffers() hands the launches that solve ("SENSOR bodies"; no sensor: nothing)
}

// One substep of the contact pipeline (neighbour lists must be current): the form the split API
// (xpbd_world_contacts_substep) exposes, with a seam for the halo exchange after it.
// awake: all bodies, or (sleeping on, from step_contacts) all but the sleepers.
int substep_contacts(xpbd_world *w, double h, uint32_t *trace, uint32_t trace_row, const xpbd::BodySubset &awake, uint32_t kinematic_left)
{
    const xpbd::BodyArrays b = w->arrays();
    const xpbd::ContactBuffers c = w->contact_buffers();
    if (kinematic_left) // before the copy below: the restitution pass sees the scripted start velocities
        XPBD_HIP_TRY(xpbd::launch_kinematic_velocities(b, w->kinematics.view(), h, kinematic_left, nullptr, w->stream));
    if (c.restitution) {
        // The velocity pass reads, of every body, the velocities the substep started from and the state after derive while it
        // writes its own body's result: the former are copied aside first (fields D_VEL.. of the SoA state are one block), the
        // latter goes to dyn_alt, and the pass writes the SoA state, which nobody reads by then.
        XPBD_HIP_TRY(hipMemcpyAsync(w->rs_start.ptr, b.dyn + (size_t)xpbd::D_VEL * b.stride, (size_t)6 * b.stride * 8, hipMemcpyDeviceToDevice,
                                    w->stream));
    }
    XPBD_HIP_TRY(xpbd::launch_integrate_ground(b, w->geom.shapes(), h, c, w->last_mask.as<uint32_t>(), trace, trace_row, w->stream, awake));
    if (int rc = narrowphase_contacts(w, b, c))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_joint_extras(h, c, w->stream));
    const xpbd::ContactBuffers solve = w->solve_buffers(c);
    if (!c.restitution) {
        XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, b.dyn, h, solve, w->stream, awake));
    } else {
        XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, w->dyn_alt.as<double>(), h, solve, w->stream, awake));
        XPBD_HIP_TRY(xpbd::launch_restitution(b, w->dyn_alt.as<double>(), w->rs_start.as<double>(), w->geom.shapes(), solve, w->last_mask.as<uint32_t>(),
                                              w->stream, awake));
    }
    // stage 7 (include/xpbd.h, "DAMPING") on the end-of-substep state, which is in the SoA arrays either way
    if (w->damping_on())
        XPBD_HIP_TRY(xpbd::launch_damping(b, w->damping_tables(), h, c, w->stream, awake));
    return XPBD_OK;
}

// One xpbd_world_step in XPBD_MODE_CONTACTS (semantics: oracle/xpbd_pairs_oracle.h).  All substeps run here, so the
// pair solve of substep k and the integrate + ground stage of substep k + 1 are one kernel; the body records alternate
// between two sets because the bodies still read each other's records of substep k while those of k + 1 are written.
// Between the substeps the state lives in the records only; the SoA arrays are read by the first kernel and written by
// the last.
int step_contacts(xpbd_world *w, double dt, double h, uint32_t substeps, uint32_t *trace)
{
    if (!w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "XPBD_MODE_CONTACTS needs xpbd_world_set_polytopes");
    // Kinematic bodies (include/xpbd.h, "KINEMATIC bodies"): the overwrite of substep 0 comes before the broadphase, whose bounding
    // spheres then include the scripted travel; with sleeping on it also tells who is MOVING in this frame.  No table: nothing.
    const bool kinematic = w->kinematics.any() && substeps != 0 && w->n != 0;
    w->sleep.moving = false;
    if (kinematic) {
        uint8_t *moving = nullptr;
        if (w->sleep.on) {
            XPBD_TRY(w->sleep.ensure(w));
            moving = w->sleep.view(w).moving;
            XPBD_HIP_TRY(hipMemsetAsync(moving, 0, w->stride, w->stream));
            w->sleep.moving = true;
        }
        XPBD_HIP_TRY(xpbd::launch_kinematic_velocities(w->arrays(), w->kinematics.view(), h, substeps, moving, w->stream));
    }
    if (int rc = build_neighbours(w, dt))
        return rc;
    if (substeps == 0)
        return XPBD_OK;
    // Sleeping (include/xpbd.h, "SLEEPING"): the sleepers' records once, every per-body stage without them, the sleep pass last.
    // Off: `awake` is the default subset and nothing else happens, the launches are the ones of a world without sleeping.
    xpbd::BodySubset awake;
    if (w->sleep.on) {
        XPBD_TRY(w->sleep.frame_records(w, trace, substeps));
        awake.skip = w->sleep.asleep(w);
    }
    // the velocity pass sits where the fused kernel below has the next substep's integrate; and that kernel has no terrain form
    // ... and the kinematic overwrite goes between the substeps, on the SoA state the fused kernel does not write, as does stage 7
    if (w->restitution.on || w->terrain.planes || kinematic || w->damping_on()) {
        for (uint32_t k = 0; k < substeps; ++k)
            if (int rc = substep_contacts(w, h, trace, k, awake, kinematic && k ? substeps - k : 0u))
                return rc;
        return w->sleep.on ? w->sleep.frame_end(w) : XPBD_OK;
    }
    XPBD_HIP_TRY(xpbd::launch_integrate_ground(w->arrays(), w->geom.shapes(), h, w->contact_buffers(0), w->last_mask.as<uint32_t>(), trace, 0,
                                               w->stream, awake));
    for (uint32_t k = 0; k < substeps; ++k) {
        const xpbd::BodyArrays b = w->arrays();
        const xpbd::ContactBuffers c = w->contact_buffers(k & 1u);
        if (int rc = narrowphase_contacts(w, b, c))
            return rc;
        XPBD_HIP_TRY(xpbd::launch_joint_extras(h, c, w->stream));
        const xpbd::ContactBuffers solve = w->solve_buffers(c);
        if (k + 1 < substeps) {
            const xpbd::ContactBuffers next = w->contact_buffers((k + 1u) & 1u);
            XPBD_HIP_TRY(xpbd::launch_pair_solve_integrate_ground(b, w->geom.shapes(), h, solve, next.rec, w->last_mask.as<uint32_t>(), trace,
                                                                  k + 1, w->stream, awake));
        } else {
            XPBD_HIP_TRY(xpbd::launch_pair_solve_derive(b, b.dyn, h, solve, w->stream, awake));
        }
    }
    return w->sleep.on ? w->sleep.frame_end(w) : XPBD_OK;
}

// ---- the frame of a multi-GPU shard, split at the halo exchange (xpbd_internal.h) -------------------------------------------
namespace xpbd {

int halo_frame_begin_enqueue(xpbd_world *w, double dt) noexcept
{
    if (!w || w->mode != XPBD_MODE_CONTACTS || !w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "halo_frame_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    return build_neighbours_enqueue(w, dt);
}

int halo_frame_begin_collect(xpbd_world *w, double h) noexcept
{
    if (!w || w->mode != XPBD_MODE_CONTACTS || !w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "halo_frame_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    if (int rc = build_neighbours_collect(w))
        return rc;
    XPBD_HIP_TRY(launch_integrate_ground(w->arrays(), w->geom.shapes(), h, w->contact_buffers(0), w->last_mask.as<uint32_t>(), nullptr, 0, w->stream));
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
    if (w->snapshot.state.bytes < dyn_bytes + mask_bytes) {
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // reserve() frees the old block
        XPBD_HIP_TRY(w->snapshot.state.reserve(dyn_bytes + mask_bytes));
    }
    char *dst = static_cast<char *>(w->snapshot.state.ptr);
    XPBD_HIP_TRY(hipMemcpyAsync(dst, w->dyn.ptr, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(dst + dyn_bytes, w->last_mask.ptr, mask_bytes, hipMemcpyDeviceToDevice, w->stream));
    w->snapshot.valid = true;
    w->snapshot.stepped = w->stepped;
    return XPBD_OK;
}

int frame_snapshot_restore(xpbd_world *w) noexcept
{
    if (!w)
        return set_error(XPBD_E_INVALID, "frame_snapshot_restore: NULL world");
    if (w->n == 0)
        return XPBD_OK;
    if (!w->snapshot.valid)
        return set_error(XPBD_E_INVALID, "frame_snapshot_restore: no snapshot");
    if (int rc = bind_device(w))
        return rc;
    const size_t dyn_bytes = (size_t)kDynFields * w->stride * 8, mask_bytes = (size_t)w->stride * 4;
    const char *src = static_cast<const char *>(w->snapshot.state.ptr);
    XPBD_HIP_TRY(hipMemcpyAsync(w->dyn.ptr, src, dyn_bytes, hipMemcpyDeviceToDevice, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(w->last_mask.ptr, src + dyn_bytes, mask_bytes, hipMemcpyDeviceToDevice, w->stream));
    w->stepped = w->snapshot.stepped;
    w->bp.have_neighbours = false;
    w->bp.pending = false;
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
        XPBD_HIP_TRY(launch_pair_solve_integrate_ground(b, w->geom.shapes(), h, c, w->contact_buffers((k + 1u) & 1u).rec, w->last_mask.as<uint32_t>(),
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
    XPBD_HIP_TRY(launch_integrate_ground(b, w->geom.shapes(), h, w->contact_buffers((k + 1u) & 1u), w->last_mask.as<uint32_t>(), nullptr, k + 1, w->stream,
                                         subset));
    return XPBD_OK;
}

} // namespace xpbd

extern "C" {

// ---- the narrowphases alone, on pairs the caller names (diagnostics) ----------------------------------------------------------
int xpbd_world_narrowphase(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_manifold *out)
try {
    static_assert(sizeof(xpbd_manifold) == sizeof(xpbd::Manifold), "xpbd_manifold must mirror xpbd::Manifold");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: NULL argument");
    if (!w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->np_staging.pairs.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->np_staging.results.reserve((size_t)n_pairs * sizeof(xpbd::Manifold)));
    XPBD_HIP_TRY(hipMemcpyAsync(w->np_staging.pairs.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->np_staging.results.ptr, 0, (size_t)n_pairs * sizeof(xpbd::Manifold), w->stream));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_sat_pairs(w->arrays(), w->geom.tables(), w->cb_rec.as<double>(), w->np_staging.pairs.as<uint32_t>(),
                                        n_pairs, w->np_staging.results.as<xpbd::Manifold>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->np_staging.results.ptr, (size_t)n_pairs * sizeof(xpbd::Manifold),
                                hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_edge_axes_separation(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_edge_query *out)
try {
    static_assert(sizeof(xpbd_edge_query) == sizeof(xpbd::EdgeQuery), "xpbd_edge_query must mirror xpbd::EdgeQuery");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: NULL argument");
    if (!w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_edge_axes_separation: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->np_staging.pairs.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->np_staging.results.reserve((size_t)n_pairs * sizeof(xpbd::EdgeQuery)));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(hipMemcpyAsync(w->np_staging.pairs.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_edge_axes_reference(w->arrays(), w->geom.tables(), w->cb_rec.as<double>(), w->np_staging.pairs.as<uint32_t>(), n_pairs,
                                                  w->np_staging.results.as<xpbd::EdgeQuery>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->np_staging.results.ptr, (size_t)n_pairs * sizeof(xpbd::EdgeQuery), hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_narrowphase_gjk(xpbd_world *w, const uint32_t *pairs, uint32_t n_pairs, xpbd_gjk_result *out)
try {
    static_assert(sizeof(xpbd_gjk_result) == sizeof(xpbd::GjkResult), "xpbd_gjk_result must mirror xpbd::GjkResult");
    if (!w || (n_pairs && (!pairs || !out)))
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: NULL argument");
    if (!w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: call xpbd_world_set_polytopes first");
    for (uint32_t k = 0; k < 2 * n_pairs; ++k)
        if (pairs[k] >= w->n)
            return set_error(XPBD_E_INVALID, "xpbd_world_narrowphase_gjk: pair %u names body %u of %u", k / 2, pairs[k], w->n);
    if (n_pairs == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    XPBD_HIP_TRY(w->np_staging.pairs.reserve((size_t)n_pairs * 8));
    XPBD_HIP_TRY(w->np_staging.results.reserve((size_t)n_pairs * sizeof(xpbd::GjkResult)));
    XPBD_HIP_TRY(w->cb_rec.reserve((size_t)xpbd::kRecDoubles * w->stride * 8));
    XPBD_HIP_TRY(hipMemcpyAsync(w->np_staging.pairs.ptr, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->np_staging.results.ptr, 0, (size_t)n_pairs * sizeof(xpbd::GjkResult), w->stream));
    XPBD_HIP_TRY(xpbd::launch_body_frames(w->arrays(), w->cb_rec.as<double>(), w->stream));
    if (int rc = w->np.ensure_gjk_scratch(n_pairs, w->stream))
        return rc;
    XPBD_HIP_TRY(xpbd::launch_gjk_epa_pairs(w->arrays(), w->geom.tables(), w->cb_rec.as<double>(),
                                            w->np_staging.pairs.as<uint32_t>(), n_pairs, w->np_staging.results.as<xpbd::GjkResult>(),
                                            nullptr, w->np.gjk_scratch, false, nullptr, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(out, w->np_staging.results.ptr, (size_t)n_pairs * sizeof(xpbd::GjkResult), hipMemcpyDeviceToHost,
                                w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

// ---- the split API ------------------------------------------------------------------------------------------------------------
int xpbd_world_contacts_begin(xpbd_world *w, double dt)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: NULL world");
    if (w->mode != XPBD_MODE_CONTACTS || !w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: needs XPBD_MODE_CONTACTS and xpbd_world_set_polytopes");
    if (w->sleep.on)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: the split API has no frame end, sleeping is on (xpbd_world_set_sleeping)");
    if (w->kinematics.any())
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_begin: the split API does not know the frame's substep count, the kinematic table is not empty "
                                         "(xpbd_world_set_kinematics)");
    if (int rc = bind_device(w))
        return rc;
    w->stepped = true;
    if (w->n == 0)
        return XPBD_OK;
    const int rc = build_neighbours(w, dt);
    if (rc)
        w->report.reset();
    return rc;
} XPBD_ABI_CATCH

int xpbd_world_contacts_substep(xpbd_world *w, double h)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: NULL world");
    if (w->mode != XPBD_MODE_CONTACTS || (w->n && !w->bp.have_neighbours))
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: call xpbd_world_contacts_begin first");
    if (w->sleep.on)
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: the split API has no frame end, sleeping is on (xpbd_world_set_sleeping)");
    if (w->kinematics.any())
        return set_error(XPBD_E_INVALID, "xpbd_world_contacts_substep: the split API does not know the frame's substep count, the kinematic table is not empty "
                                         "(xpbd_world_set_kinematics)");
    if (w->n == 0)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    const int rc = substep_contacts(w, h, nullptr, 0);
    if (rc)
        w->report.reset();
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
    w->np.sat_schedule = schedule;
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
    w->sleep.wake_all(true);
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
    out[0] = w->bp.n_pairs;
    out[1] = out[2] = 0;
    if (!w->np.stats.ptr)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    unsigned long long host[2] = {0, 0};
    XPBD_HIP_TRY(hipMemcpyAsync(host, w->np.stats.ptr, 16, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemsetAsync(w->np.stats.ptr, 0, 16, w->stream));
    w->np.stats_touching_seen = 0; // the schedule heuristic of build_neighbours starts counting afresh
    w->np.stats_pair_substeps_seen = w->np.stats_pair_substeps;
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    out[1] = host[0];
    out[2] = host[1];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_build_neighbours(xpbd_world *w, double dt, uint32_t *n_entries_out)
try {
    if (!w || !n_entries_out)
        return set_error(XPBD_E_INVALID, "xpbd_world_build_neighbours: NULL argument");
    if (!w->geom.has_topology)
        return set_error(XPBD_E_INVALID, "xpbd_world_build_neighbours: call xpbd_world_set_polytopes first");
    if (w->sleep.on) // (a broadphase applies the pending wake requests, which belongs to the start of a step)
        return set_error(XPBD_E_INVALID, "xpbd_world_build_neighbours: a broadphase outside a step, sleeping is on (xpbd_world_set_sleeping)");
    if (int rc = bind_device(w))
        return rc;
    if (int rc = build_neighbours(w, dt))
        return rc;
    *n_entries_out = w->bp.n_entries;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_neighbours(xpbd_world *w, uint32_t *offsets, uint32_t *neighbours, uint32_t cap)
try {
    if (!w || !offsets || (!neighbours && cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_neighbours: NULL argument");
    if (!w->bp.have_neighbours)
        return set_error(XPBD_E_INVALID, "xpbd_world_download_neighbours: no neighbour lists built yet");
    if (cap < w->bp.n_entries)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_neighbours: %u entries, capacity %u", w->bp.n_entries, cap);
    if (int rc = bind_device(w))
        return rc;
    XPBD_HIP_TRY(hipMemcpyAsync(offsets, w->bp.nbr_off.ptr, (size_t)(w->n + 1) * 4, hipMemcpyDeviceToHost, w->stream));
    if (w->bp.n_entries)
        XPBD_HIP_TRY(hipMemcpyAsync(neighbours, w->bp.nbr.ptr, (size_t)w->bp.n_entries * 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

} // extern "C"
