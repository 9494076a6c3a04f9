// xpbd_world_sensors.cpp -- sensor bodies of the single-GPU world: Sensors (xpbd_world.hpp), the five entry points, and the
// three things the rest of the world asks of the unit -- the masked pair codes behind a narrowphase (narrowphase_contacts), the
// contact edges without the sensor pairs (Islands::enqueue, Sleep::frame_end) and "a sensor is not inert" (Sleep::frame_begin).
// Semantics: include/xpbd.h, "SENSOR bodies"; the kernels: xpbd_sensors.hip.
#include <cstring>
#include <vector>

#include "xpbd_world.hpp"
#include "xpbd_checks.hpp"
#include "xpbd_scan.h"

namespace {

xpbd::SensorTarget sensor_target(const xpbd_world *w)
{
    return xpbd::SensorTarget{w->n, w->sensors.count, w->report.on, w->report.frame && w->report.substeps != 0};
}

// Both variants of the occupancy after their checks: everything enqueued on the world's stream, into device arrays.
int enqueue_overlaps(xpbd_world *w, uint32_t *dev_sensors, uint32_t *dev_offsets, xpbd_sensor_hit *dev_hits, uint32_t cap)
{
    Sensors &s = w->sensors;
    ContactReport &r = w->report;
    const size_t n = w->n;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{s.list, (size_t)s.count * 4},
                                                      {s.list_flag, (n + 1) * 4},
                                                      {s.occ_scan, xpbd::scan_scratch_bytes(n)}}));
    if (!s.list_ready) { // once per table
        XPBD_HIP_TRY(xpbd::launch_sensor_list(s.flags.as<uint8_t>(), w->n, s.list_flag.as<uint32_t>(), s.occ_scan.as<uint32_t>(), s.list.as<uint32_t>(),
                                              w->stream));
        s.list_ready = true;
    }
    if (!r.keys_ready) // the scanned key flags name every touching pair's record
        XPBD_TRY(r.compact_keys(w));
    const xpbd::SensorFrame f{s.list.as<uint32_t>(), s.count, w->bp.nbr_off.as<uint32_t>(), w->bp.nbr.as<uint32_t>(), w->bp.nbr_pair.as<uint32_t>(),
                              r.touch.as<uint32_t>(), r.flag.as<uint32_t>()};
    XPBD_HIP_TRY(xpbd::launch_sensor_overlaps(f, dev_sensors, dev_offsets, dev_hits, cap, s.occ_scan.as<uint32_t>(), w->stream));
    return XPBD_OK;
}

} // namespace

int contact_edge_keys(xpbd_world *w, const unsigned long long **keys, const uint32_t **key_count)
{
    ContactReport &r = w->report;
    if (!r.keys_ready)
        XPBD_TRY(r.compact_keys(w));
    *keys = r.keys[r.cur].as<unsigned long long>();
    *key_count = r.flag.as<uint32_t>() + w->bp.n_pairs;
    Sensors &s = w->sensors;
    if (!s.any())
        return XPBD_OK;
    const size_t lanes = w->bp.n_pairs;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{s.key_flag, (lanes + 1) * 4}, {s.key_scan, xpbd::scan_scratch_bytes(lanes)}, {s.solid_keys, lanes * 8}}));
    XPBD_HIP_TRY(xpbd::launch_sensor_solid_keys(*keys, *key_count, w->bp.n_pairs, s.flags.as<uint8_t>(), s.key_flag.as<uint32_t>(), s.key_scan.as<uint32_t>(),
                                                s.solid_keys.as<unsigned long long>(), w->stream));
    *keys = s.solid_keys.as<unsigned long long>();
    *key_count = s.key_flag.as<uint32_t>() + w->bp.n_pairs;
    return XPBD_OK;
}

int sensor_mask_codes(xpbd_world *w, const xpbd::ContactBuffers &c)
{
    Sensors &s = w->sensors;
    if (!s.any() || w->bp.n_pairs == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{s.solve_codes, (size_t)w->bp.n_pairs}}));
    XPBD_HIP_TRY(xpbd::launch_sensor_mask_codes(c.pairs, s.flags.as<uint8_t>(), c.pair_codes, s.solve_codes.as<uint8_t>(), w->bp.n_pairs, w->stream));
    return XPBD_OK;
}

int sensor_not_inert(xpbd_world *w)
{
    if (!w->sensors.any())
        return XPBD_OK;
    XPBD_HIP_TRY(xpbd::launch_sensor_not_inert(w->sensors.flags.as<uint8_t>(), w->sleep.view(w).inert, w->n, w->stream));
    return XPBD_OK;
}

extern "C" {

int xpbd_world_set_sensors(xpbd_world *w, const uint8_t *is_sensor, uint32_t n)
try {
    const char *who = "xpbd_world_set_sensors";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    uint32_t count = 0;
    XPBD_TRY(sensor_target(w).table_check(who, is_sensor, n, false, &count));
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // queued substeps may still read the present table
    if (!is_sensor || n == 0) {
        w->sleep.wake_all(true);
        w->sensors.clear();
        return XPBD_OK;
    }
    std::vector<uint8_t> host(is_sensor, is_sensor + n);
    XPBD_TRY(upload_table(w->sensors.flags, is_sensor, n));
    w->sleep.wake_all(true); // nothing can fail any more
    w->sensors.host.swap(host);
    w->sensors.count = count;
    w->sensors.list_ready = false;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_get_sensors(xpbd_world *w, uint8_t *is_sensor, uint32_t n)
try {
    const char *who = "xpbd_world_get_sensors";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sensor_target(w).table_check(who, is_sensor, n, true));
    if (n == 0)
        return XPBD_OK;
    if (w->sensors.host.size() == n)
        std::memcpy(is_sensor, w->sensors.host.data(), n);
    else
        std::memset(is_sensor, 0, n);
    return XPBD_OK;
} XPBD_ABI_CATCH

uint32_t xpbd_world_sensor_count(const xpbd_world *w) noexcept { return w ? w->sensors.count : 0u; }

int xpbd_world_sensor_overlaps(xpbd_world *w, uint32_t *sensors, uint32_t *offsets, xpbd_sensor_hit *hits, uint32_t cap, uint32_t *n_out)
try {
    const char *who = "xpbd_world_sensor_overlaps";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sensor_target(w).overlaps_check(who, sensors, offsets, hits, cap, n_out, true));
    XPBD_TRY(bind_device(w));
    Sensors &s = w->sensors;
    const uint32_t count = s.count;
    const uint32_t room = cap < w->bp.n_entries ? cap : w->bp.n_entries; // (no sensor has more hits than the lists have entries)
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{s.occ_sensors, (size_t)count * 4},
                                                      {s.occ_offsets, ((size_t)count + 1) * 4},
                                                      {s.occ_hits, (size_t)at_least_one(room) * sizeof(xpbd_sensor_hit)}}));
    XPBD_TRY(enqueue_overlaps(w, s.occ_sensors.as<uint32_t>(), s.occ_offsets.as<uint32_t>(), s.occ_hits.as<xpbd_sensor_hit>(), room));
    XPBD_HIP_TRY(hipMemcpyAsync(sensors, s.occ_sensors.ptr, (size_t)count * 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(offsets, s.occ_offsets.ptr, ((size_t)count + 1) * 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = offsets[count], take = total < room ? total : room;
    *n_out = total;
    if (take) {
        XPBD_HIP_TRY(hipMemcpyAsync(hits, s.occ_hits.ptr, (size_t)take * sizeof(xpbd_sensor_hit), hipMemcpyDeviceToHost, w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "%s: %u hits, capacity %u", who, total, cap);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_sensor_overlaps_device(xpbd_world *w, uint32_t *dev_sensors, uint32_t *dev_offsets, xpbd_sensor_hit *dev_hits, uint32_t cap)
try {
    const char *who = "xpbd_world_sensor_overlaps_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sensor_target(w).overlaps_check(who, dev_sensors, dev_offsets, dev_hits, cap, nullptr, false));
    XPBD_TRY(bind_device(w));
    return enqueue_overlaps(w, dev_sensors, dev_offsets, dev_hits, cap);
} XPBD_ABI_CATCH

} // extern "C"
