// xpbd_world_islands.cpp -- contact islands of the single-GPU world: Islands (xpbd_world.hpp) and the island entry points.
// Semantics: include/xpbd.h, "Contact ISLANDS"; the kernels: xpbd_islands.hip.
#include "xpbd_world.hpp"
#include "xpbd_scan.h"

namespace {

xpbd::IslandsTarget islands_target(const xpbd_world *w)
{
    return xpbd::IslandsTarget{w->n, w->report.on, w->report.frame && w->report.substeps != 0};
}

} // namespace

// Room for one call.  Queued work (an earlier call) may still use the scratch: the stream is waited for only when a buffer
// has to grow.  host_island_of / host_records: the staging of the host variant's outputs.
int Islands::reserve(const xpbd_world *w, bool host_island_of, uint32_t host_records)
{
    const size_t n = w->n;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{parent, n * 4},
                                                      {fixed, n},
                                                      {flag, (n + 1) * 4},
                                                      {scan, xpbd::scan_scratch_bytes(n)},
                                                      {result, 2 * sizeof(uint32_t)},
                                                      {island_of, host_island_of ? n * 4 : 0},
                                                      {records, (size_t)host_records * sizeof(xpbd_island)}}));
    return XPBD_OK;
}

// The whole pass, enqueued only.  The contact edges are the report's keys of the current frame: compacted now if they are not
// (enqueued only, as the report's own frame_end does), their count read where the scan left it on the device.
int Islands::enqueue(xpbd_world *w, uint32_t flags, uint32_t *dev_island_of, xpbd_island *dev_records, uint32_t cap, uint32_t *dev_total)
{
    xpbd::IslandsWork k{};
    k.dyn = w->dyn.as<double>();
    k.stat = w->stat.as<double>();
    k.stride = w->stride;
    k.n = w->n;
    k.last_mask = w->last_mask.as<uint32_t>();
    if (!(flags & XPBD_ISLANDS_NO_CONTACTS) && w->bp.n_pairs) {
        XPBD_TRY(contact_edge_keys(w, &k.keys, &k.key_count)); // (without the sensor pairs: "SENSOR bodies")
        k.key_lanes = w->bp.n_pairs;
    }
    if (!(flags & XPBD_ISLANDS_NO_JOINTS) && w->joints.csr.n) {
        k.joints = w->joints.csr.joints.as<xpbd::Joint>();
        k.n_joints = w->joints.csr.n;
    }
    k.parent = parent.as<uint32_t>();
    k.fixed = fixed.as<uint8_t>();
    k.flag = flag.as<uint32_t>();
    k.scan = scan.as<uint32_t>();
    k.status = result.as<uint32_t>();
    XPBD_HIP_TRY(xpbd::launch_islands(k, dev_island_of, dev_records, cap, dev_total, w->stream));
    return XPBD_OK;
}

extern "C" {

int xpbd_world_islands(xpbd_world *w, uint32_t flags, uint32_t *island_of, xpbd_island *islands, uint32_t cap, uint32_t *n_islands)
try {
    const char *who = "xpbd_world_islands";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(islands_target(w).check(who, flags, islands, cap, n_islands));
    XPBD_TRY(bind_device(w));
    Islands &s = w->islands;
    const uint32_t room = cap < w->n ? cap : w->n; // (there are at most as many islands as bodies)
    XPBD_TRY(s.reserve(w, island_of != nullptr, room));
    uint32_t *dev_result = s.result.as<uint32_t>();
    XPBD_TRY(s.enqueue(w, flags, island_of ? s.island_of.as<uint32_t>() : nullptr, room ? s.records.as<xpbd_island>() : nullptr, room,
                       dev_result + 1));
    uint32_t result[2] = {0u, 0u}; // the give-up word, the island count
    XPBD_HIP_TRY(hipMemcpyAsync(result, dev_result, sizeof result, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    if (result[0] || result[1] > w->n)
        return set_error(XPBD_E_HIP, "%s: the grouping of %u bodies ran into its loop bound (give-up word %u, count %u)", who, w->n, result[0],
                         result[1]);
    const uint32_t total = result[1], take = total < cap ? total : cap;
    *n_islands = total;
    if (island_of)
        XPBD_HIP_TRY(hipMemcpyAsync(island_of, s.island_of.ptr, (size_t)w->n * 4, hipMemcpyDeviceToHost, w->stream));
    if (take)
        XPBD_HIP_TRY(hipMemcpyAsync(islands, s.records.ptr, (size_t)take * sizeof(xpbd_island), hipMemcpyDeviceToHost, w->stream));
    if (island_of || take)
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "%s: %u islands, capacity %u", who, total, cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_islands_device(xpbd_world *w, uint32_t flags, uint32_t *dev_island_of, xpbd_island *dev_islands, uint32_t cap,
                              uint32_t *dev_n_islands)
try {
    const char *who = "xpbd_world_islands_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(islands_target(w).check(who, flags, dev_islands, cap, dev_n_islands));
    XPBD_TRY(bind_device(w));
    XPBD_TRY(w->islands.reserve(w, false, 0));
    return w->islands.enqueue(w, flags, dev_island_of, dev_islands, cap, dev_n_islands);
} XPBD_ABI_CATCH

} // extern "C"
