// xpbd_sensors.h -- SENSOR bodies (EXTENSION): launchers for xpbd_sensors.hip.  Semantics: include/xpbd.h, "SENSOR bodies".
//
// A sensor is a body flagged in a per-body byte table (0 / 1).  Nothing here touches a kernel of another unit: the narrowphase
// and the report keep the pair codes as they are; the pair solve and restitution are handed a MASKED copy (code 0 for a pair
// with a sensor end); islands and sleeping are handed the report's keys without the sensor pairs; the broadphase sees a sensor
// as not inert.  Occupancy (who touched which sensor in the frame) walks the sensors' neighbour lists, which the broadphase left
// ascending.  Integers only; every position comes from a scan or a ballot, never from an atomic.
#pragma once

#include "xpbd_kernels.h"

namespace xpbd {

// solve_codes[p] = (sensor[a] | sensor[b]) ? 0 : codes[p] for the n_pairs pairs (a, b) of `pairs`.
hipError_t launch_sensor_mask_codes(const uint32_t *pairs, const uint8_t *sensor, const uint8_t *codes, uint8_t *solve_codes, uint32_t n_pairs,
                                    hipStream_t stream);

// The keys (a << 32 | b, ascending, *key_count <= key_lanes of them) without those that have a sensor end, in order: flag
// ([key_lanes + 1], scanned in place: flag[key_lanes] = how many are kept), scratch (launch_exclusive_scan's), out [key_lanes].
hipError_t launch_sensor_solid_keys(const unsigned long long *keys, const uint32_t *key_count, uint32_t key_lanes, const uint8_t *sensor, uint32_t *flag,
                                    uint32_t *scratch, unsigned long long *out, hipStream_t stream);

// inert[i] = 0 for every sensor i < n (behind launch_sleep_frame_begin).
hipError_t launch_sensor_not_inert(const uint8_t *sensor, uint8_t *inert, uint32_t n, hipStream_t stream);

// The sensors' indices, ascending: flag ([n + 1], scanned in place: flag[n] = their number), scratch, list [that number].
hipError_t launch_sensor_list(const uint8_t *sensor, uint32_t n, uint32_t *flag, uint32_t *scratch, uint32_t *list, hipStream_t stream);

// A per-body flag table across a population change: fresh[s] = old[src[s]] for s < n_keep (src == NULL: old[s]), 0 for
// n_keep <= s < n_new.
hipError_t launch_sensor_gather(const uint8_t *old, uint8_t *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, hipStream_t stream);

// What the occupancy reads of the current report frame.
struct SensorFrame {
    const uint32_t *list;      // [n_sensors] ascending body indices (launch_sensor_list)
    uint32_t n_sensors;
    const uint32_t *nbr_off;   // the broadphase's neighbour lists, ascending per body, and the pair of every entry
    const uint32_t *nbr;
    const uint32_t *nbr_pair;
    const uint32_t *touch;     // [n_pairs] substeps of the frame in which the pair touched (xpbd_report.h)
    const uint32_t *record_of; // [n_pairs] the report's scanned key flags: the index of a touching pair's record
};
// sensors[k] = list[k]; offsets[0..n_sensors]: hits[offsets[k] .. offsets[k + 1]) = the neighbours of sensor k whose pair
// touched, in neighbour order, with their record; only the first `cap` hits are written, offsets[n_sensors] is the total.
// scratch: launch_exclusive_scan's for n_sensors entries.  One wave per sensor.
hipError_t launch_sensor_overlaps(const SensorFrame &f, uint32_t *sensors, uint32_t *offsets, xpbd_sensor_hit *hits, uint32_t cap, uint32_t *scratch,
                                  hipStream_t stream);

} // namespace xpbd
