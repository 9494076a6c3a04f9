// xpbd_internal.h -- shared by the translation units behind the C ABI (not installed).
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "xpbd_checks.hpp" // the argument checks both worlds share
#include "xpbd_error.h"
#include "xpbd_shape_tables.hpp" // the compiler of the shape tables, for both worlds too

namespace xpbd {

// ---- host resource layer (the error layer: xpbd_error.h) ---------------------------------------------------------------------
#define XPBD_HIP_TRY(expr)                                                                                       \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return ::xpbd::set_error(e_ == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "%s failed: %s", #expr,   \
                                     hipGetErrorString(e_));                                                        \
    } while (0)

// A device allocation that only ever grows, freed with its owner.  The first request is served exactly (most buffers are
// sized by the body count and never change); a buffer that has to GROW takes a quarter more than asked: the pair, neighbour
// and manifold buffers follow the pair count of the frame, which creeps up frame after frame while a pile settles, the ghost
// lists of the multi-GPU world grow with the re-plans, and every hipFree + hipMalloc of a block of ~100 MB stalls the stream
// for several hundred microseconds.  Growing frees the old block: queued work must not use it any more.
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;

    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        std::swap(ptr, o.ptr);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DeviceBuffer() { release(); }

    hipError_t reserve(size_t want) noexcept
    {
        if (want <= bytes)
            return hipSuccess;
        if (ptr) {
            want += want / 4;
            hipError_t e = hipFree(ptr);
            ptr = nullptr;
            bytes = 0;
            if (e != hipSuccess)
                return e;
        }
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess)
            bytes = want;
        return e;
    }
    void release() noexcept
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};

// Room in buffers that work queued on `stream` may still use: growing one frees its block, so the stream is waited for first --
// only when one of them has to grow.
struct Reservation {
    DeviceBuffer &buffer;
    size_t bytes;
};
inline hipError_t reserve_after_sync(hipStream_t stream, std::initializer_list<Reservation> need) noexcept
{
    bool grow = false;
    for (const Reservation &r : need)
        grow = grow || r.buffer.bytes < r.bytes;
    if (!grow)
        return hipSuccess;
    hipError_t e = hipStreamSynchronize(stream);
    for (const Reservation &r : need)
        if (e == hipSuccess)
            e = r.buffer.reserve(r.bytes);
    return e;
}

// ---- one frame of a shard of the multi-GPU world (xpbd_multi.cpp), split at the halo exchange ---------------------------
// All device pointers; slots are local body indices of the shard's world.
struct HaloLists {
    const uint32_t *boundary;   // owned bodies that other ranks mirror (ascending)
    uint32_t n_boundary;
    const uint32_t *ghosts;     // local copies of remote bodies (ascending)
    const uint32_t *ghost_rows; // their rows in the gathered buffer
    uint32_t n_ghosts;
    const uint8_t *skip;        // [n] 1 for boundary and ghost bodies: what the interior launch leaves out (NULL: none)
    double *send;               // n_boundary rows of 13 doubles: this shard's contribution to the all-gather
    const double *recv;         // the gathered buffer
};

} // namespace xpbd

struct xpbd_world;
struct xpbd_joint;
struct xpbd_joint_limit;
struct xpbd_joint_drive;
struct xpbd_material;
struct xpbd_ray;
struct xpbd_impulse;
struct xpbd_ray_hit;
struct xpbd_overlap_query;
struct xpbd_overlap_hit;
struct xpbd_sweep;
struct xpbd_sweep_hit;
struct xpbd_distance_query;
struct xpbd_distance_hit;
struct xpbd_pair_contact;
struct xpbd_contact_point;

namespace xpbd {
// frame:   halo_frame_begin_enqueue; halo_frame_begin_collect; substeps x { halo_substep_boundary; <all-gather send -> recv,
//          overlapping:> halo_substep_interior; <wait for the gather> halo_substep_ghosts }
// begin:    the broadphase of the frame and the integrate + ground stage of substep 0 for every local body, in two halves
//           (enqueue = bounding spheres, buckets, neighbour counts, the totals on their way to pinned host memory, no wait;
//           collect = wait for the totals, size the pair buffers, fill the lists, integrate + ground stage of substep 0)
// boundary: the narrowphase of substep k, then the pair solve (+ the integrate + ground stage of substep k + 1 unless `last`)
//           of the BOUNDARY bodies, whose end-of-substep state goes straight into `send`
// interior: the same for the owned bodies nobody mirrors
// ghosts:   the ghosts take their owners' end-of-substep state from `recv` (and run their own integrate + ground stage of
//           substep k + 1 unless `last`)
// Same arithmetic per body as xpbd_world_step, so the same bits.
int halo_frame_begin_enqueue(xpbd_world *w, double dt) noexcept;
int halo_frame_begin_collect(xpbd_world *w, double h) noexcept;
// The state a frame starts from (13 dynamic fields per body + last contact masks) kept aside on the device / put back:
// a frame whose halos turn out to have been too thin is undone, re-planned and run again (xpbd_multi.cpp).
int frame_snapshot_save(xpbd_world *w) noexcept;
int frame_snapshot_restore(xpbd_world *w) noexcept;
int halo_substep_boundary(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept;
int halo_substep_interior(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept;
int halo_substep_ghosts(xpbd_world *w, double h, uint32_t k, bool last, const HaloLists &l) noexcept;
// ---- a plan of the multi-GPU world with the bodies staying on the device -----------------------------------------------------
// host_keys[k] = grid cell (xpbd_halo_cell_key: same bits) of the bounding-sphere centre of body dev_slots[k] (a device array;
// NULL: body k); *bad_index = first k whose centre is not finite (UINT32_MAX: none).  Synchronous.
int halo_cell_keys(xpbd_world *w, const uint32_t *dev_slots, uint32_t n, double edge, int64_t *host_keys, uint32_t *bad_index);
// out39[k] = the xpbd_rigid of body host_slots[k] (38 doubles) and its shape id as a double.  Synchronous.
int download_records(xpbd_world *w, const uint32_t *host_slots, uint32_t n, double *out39);
// The world's bodies become: body s = the present body host_src[s] (>= 0) or incoming record -host_src[s] - 1 (39 doubles
// each).  Only the incoming records cross the bus; otherwise as xpbd_world_upload_bodies (joints and neighbour lists dropped).
int repack_bodies(xpbd_world *w, const int32_t *host_src, uint32_t n_new, const double *incoming39, uint32_t n_incoming);
// Compiled shape tables (xpbd_shape_tables.hpp) become the world's: what both shape setters end in, and how every shard takes
// tables compiled once.  A refusal (fewer shapes than the resident bodies use) or a failure leaves the previous tables in force.
int install_shape_tables(xpbd_world *w, const ShapeTablesHost &tables);
// Ray casts of the world's bodies, stream-ordered (device arrays) / from and to host arrays (waits).  dev_global_id: device
// array of w's body count, the index each body is known by (XPBD_NO_HIT: the body does not answer); NULL: its slot.
// masked: only bodies whose collision-filter group meets `mask` answer (xpbd_world_raycast_masked); else every body does.
int raycast_enqueue(xpbd_world *w, const xpbd_ray *dev_rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *dev_hits, const uint32_t *dev_global_id,
                    bool masked, uint32_t mask);
int raycast_host(xpbd_world *w, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits, const uint32_t *dev_global_id,
                 bool masked, uint32_t mask);
// Overlap queries against the world's bodies (include/xpbd.h, "Overlap queries"), stream-ordered (device arrays; the total is
// dev_offsets[n_queries]) / from and to host arrays (waits; *n_out = the total, XPBD_E_CAPACITY when it exceeds cap; a world
// without bodies reports nothing).  dev_global_id as for the ray casts: what hit.body and ignore_body mean, ascending with the slot.
int overlap_enqueue(xpbd_world *w, const xpbd_overlap_query *dev_queries, uint32_t n_queries, uint32_t flags, uint32_t *dev_offsets,
                    xpbd_overlap_hit *dev_hits, uint32_t cap, const uint32_t *dev_global_id);
int overlap_host(xpbd_world *w, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets, xpbd_overlap_hit *hits,
                 uint32_t cap, uint32_t *n_out, const uint32_t *dev_global_id);
// Sweep queries against the world's bodies (include/xpbd.h, "Sweep queries"): stream-ordered / from and to host arrays, on the
// scratch and staging of the other queries.
int sweep_enqueue(xpbd_world *w, const xpbd_sweep *dev_sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *dev_hits,
                  const uint32_t *dev_global_id);
int sweep_host(xpbd_world *w, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits, const uint32_t *dev_global_id);
// Distance queries against the world's bodies (include/xpbd.h, "Distance queries"): stream-ordered / from and to host arrays, on
// the scratch and staging of the other queries.
int distance_enqueue(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *dev_hits,
                     const uint32_t *dev_global_id);
int distance_host(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits,
                  const uint32_t *dev_global_id);
// Distance queries against the world's terrain (include/xpbd.h, "Terrain in the distance queries"): one kernel that needs no
// scratch, so the stream-ordered form never waits; the host form goes through the staging of the other queries.
int terrain_distance_enqueue(xpbd_world *w, const xpbd_distance_query *dev_queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *dev_hits);
int terrain_distance_host(xpbd_world *w, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits);
// The current frame's contact report of a shard of the multi-GPU world (include/xpbd.h, "Contact REPORTS"): only the pairs whose
// lower body has dev_owned[slot] != 0, bodies named by dev_global_id[slot] (device arrays of the world's body count; global ids
// ascending with the slot).  Waits.  A world without bodies reports nothing.
int report_shard(xpbd_world *w, const uint8_t *dev_owned, const uint32_t *dev_global_id, std::vector<xpbd_pair_contact> &pairs,
                 std::vector<xpbd_contact_point> &points) noexcept;
} // namespace xpbd
