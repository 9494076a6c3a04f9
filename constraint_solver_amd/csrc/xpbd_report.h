// xpbd_report.h -- contact REPORTS (EXTENSION): launchers for xpbd_report.hip.  Semantics: include/xpbd.h, "Contact REPORTS".
//
// Per substep one lane per pair counts the substeps in which the pair touched (touch[p], zeroed by the owner whenever the
// broadphase sizes a new pair list).  A frame's report is then compacted by scans, never by atomics: flag touch > 0, scan,
// write the sorted keys (a << 32 | b: the pair list is sorted by (a, b), so compaction keeps the order); a scan over the last
// substep's point counts places the points; the events binary-search each frame's keys in the other frame's.
#pragma once

#include "xpbd_pairs.h"

namespace xpbd {

// The pair list of one frame as the contact pipeline left it after its last substep.
struct ReportFrame {
    const uint32_t *pairs;             // [n_pairs][2], a < b, sorted by (a, b)
    const uint8_t *codes;              // [n_pairs] n_points | feature << 4 of the last substep
    const ContactManifold *manifolds;  // [n_pairs] of the last substep
    const uint32_t *touch;             // [n_pairs] substeps of the frame in which the pair touched
    uint32_t n_pairs;
    // A shard of the multi-GPU world: only pairs whose LOWER body has owned[a] != 0 (that shard holds the other body too, owned
    // or as a ghost), keys and records in global_id[slot].  Ascending global ids per slot keep the keys sorted.  NULL: all, slots.
    const uint8_t *owned;
    const uint32_t *global_id;
};

// touch[p] += (codes[p] & 0xF) != 0
hipError_t launch_report_touch(const uint8_t *codes, uint32_t *touch, uint32_t n_pairs, hipStream_t stream);
// flag: n_pairs + 1 entries, scanned in place (flag[n_pairs] = number of touching pairs K, of the owned ones in a shard); then keys[s], sel[s] (pair index)
// and npts[s] (points of the last substep) for s < K.  scratch: >= n_pairs / 1024 + 2 entries.
hipError_t launch_report_keys(const ReportFrame &f, uint32_t *flag, uint32_t *scratch, unsigned long long *keys, uint32_t *sel,
                              uint32_t *npts, hipStream_t stream);
// The K pair records (first_point: npts scanned) and, with points != NULL, their points.
hipError_t launch_report_records(const ReportFrame &f, const unsigned long long *keys, const uint32_t *sel, const uint32_t *first_point,
                                 uint32_t k, xpbd_pair_contact *out, xpbd_contact_point *points, hipStream_t stream);
// Events of cur (this frame's keys) against prev.  Flags: n_cur + n_prev + 1 entries, entry s < n_cur = key cur[s] is not in
// prev (BEGIN), entry n_cur + s = prev[s] is not in cur (END), scanned in place: flag[n_cur] = BEGINs, flag[n_cur + n_prev] =
// all events.  Write: the events into out[flag[s]] -- BEGINs then ENDs, each in key order.
hipError_t launch_report_event_flags(const unsigned long long *cur, uint32_t n_cur, const unsigned long long *prev, uint32_t n_prev,
                                     uint32_t *flag, uint32_t *scratch, hipStream_t stream);
hipError_t launch_report_event_write(const unsigned long long *cur, uint32_t n_cur, const unsigned long long *prev, uint32_t n_prev,
                                     const uint32_t *flag, xpbd_contact_event *out, hipStream_t stream);

} // namespace xpbd
