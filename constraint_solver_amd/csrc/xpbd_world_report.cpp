// xpbd_world_report.cpp -- contact reports of the single-GPU world: ContactReport (xpbd_world.hpp), the report entry points and
// the report of a shard of the multi-GPU world.  Semantics: include/xpbd.h, "Contact REPORTS".
#include <vector>

#include "xpbd_world.hpp"
#include "xpbd_scan.h"

// This frame's touching pairs -> keys[cur]; their count travels to host[cur].  Enqueued only.
int ContactReport::compact_keys(const xpbd_world *w)
{
    XPBD_HIP_TRY(xpbd::launch_report_keys(frame_of(w->bp), flag.as<uint32_t>(), scan.as<uint32_t>(), keys[cur].as<unsigned long long>(),
                                          sel.as<uint32_t>(), npts.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&host[cur], flag.as<uint32_t>() + w->bp.n_pairs, 4, hipMemcpyDeviceToHost, w->stream));
    keys_ready = true;
    return XPBD_OK;
}

// Before a broadphase replaces the pair list: the frame's touching set becomes the next frame's S_prev (a frame without a
// substep touched nothing).  The keys must be compacted now -- the pairs, codes and counters they come from are rebuilt.
int ContactReport::frame_end(const xpbd_world *w)
{
    if (!on)
        return XPBD_OK;
    if (frame && substeps) {
        if (!keys_ready)
            XPBD_TRY(compact_keys(w));
        prev_valid = true;
        cur ^= 1u;
    } else {
        prev_valid = false; // a frame without a substep touched nothing; and after an enable, upload, restore or failure S_prev is empty
    }
    frame = keys_ready = ready = false;
    substeps = 0;
    return XPBD_OK;
}

// After the broadphase has sized the pair list: the counters of the new frame start at zero.
int ContactReport::frame_begin(const xpbd_world *w)
{
    if (!on)
        return XPBD_OK;
    const size_t np = at_least_one(w->bp.n_pairs);
    XPBD_HIP_TRY(touch.reserve(np * 4));
    XPBD_HIP_TRY(flag.reserve((np + 1) * 4));
    XPBD_HIP_TRY(sel.reserve(np * 4));
    XPBD_HIP_TRY(npts.reserve((np + 1) * 4));
    XPBD_HIP_TRY(keys[cur].reserve(np * 8)); // (the other one holds S_prev)
    XPBD_HIP_TRY(scan.reserve(xpbd::scan_scratch_bytes(np)));
    XPBD_HIP_TRY(hipMemsetAsync(touch.ptr, 0, np * 4, w->stream));
    frame = true;
    keys_ready = ready = false;
    substeps = 0;
    return XPBD_OK;
}

// A substep's narrowphase has left its per-pair codes: the pairs that touch count it.
int ContactReport::note_substep(const xpbd_world *w, const uint8_t *pair_codes)
{
    if (!frame)
        return XPBD_OK;
    XPBD_HIP_TRY(xpbd::launch_report_touch(pair_codes, touch.as<uint32_t>(), w->bp.n_pairs, w->stream));
    ++substeps;
    keys_ready = ready = false;
    return XPBD_OK;
}

// Everything a count or download needs of the current frame: keys, point offsets, event flags and their totals.  Waits.
int ContactReport::prepare(const xpbd_world *w, const char *who)
{
    if (!on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_world_set_contact_report)", who);
    if (!frame || !substeps)
        return set_error(XPBD_E_INVALID, "%s: no report: no substep of XPBD_MODE_CONTACTS has run since the last broadphase, upload, "
                                         "history restore, enable, failed step or step in another mode", who);
    if (ready)
        return XPBD_OK;
    if (int rc = bind_device(w))
        return rc;
    if (!keys_ready)
        XPBD_TRY(compact_keys(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // (also: reserve() frees a block only when no queued work uses it)
    const uint32_t k = host[cur], n_prev = prev_valid ? host[cur ^ 1u] : 0u;
    const size_t n_ev = (size_t)k + n_prev;
    XPBD_HIP_TRY(ev_flag.reserve((n_ev + 1) * 4));
    XPBD_HIP_TRY(scan.reserve(xpbd::scan_scratch_bytes(n_ev))); // both scans below: k <= n_ev
    XPBD_HIP_TRY(xpbd::launch_exclusive_scan(npts.as<uint32_t>(), k, scan.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(xpbd::launch_report_event_flags(keys[cur].as<unsigned long long>(), k, keys[cur ^ 1u].as<unsigned long long>(), n_prev,
                                                 ev_flag.as<uint32_t>(), scan.as<uint32_t>(), w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&host[2], npts.as<uint32_t>() + k, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&host[3], ev_flag.as<uint32_t>() + k, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipMemcpyAsync(&host[4], ev_flag.as<uint32_t>() + n_ev, 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    counts[0] = k;
    counts[1] = host[2];
    counts[2] = host[3];
    counts[3] = host[4] - host[3];
    ready = true;
    return XPBD_OK;
}

extern "C" {

int xpbd_world_set_contact_report(xpbd_world *w, uint32_t enable)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_report: NULL world");
    if (enable > 1u)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_report: enable must be 0 or 1, not %u", enable);
    if (!enable && w->sleep.on)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_contact_report: sleeping is on and takes its touching pairs from the report "
                                         "(xpbd_world_set_sleeping(w, NULL) first)");
    if (int rc = bind_device(w))
        return rc;
    if (enable && !w->report.host)
        XPBD_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->report.host), 8 * sizeof(uint32_t), hipHostMallocDefault));
    if (!enable && w->report.on) { // (queued work may still read the buffers)
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
        w->report.release_buffers();
    }
    w->report.reset();
    w->report.on = enable != 0;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_contact_report_counts(xpbd_world *w, uint32_t out[4])
try {
    if (!w || !out)
        return set_error(XPBD_E_INVALID, "xpbd_world_contact_report_counts: NULL argument");
    XPBD_TRY(w->report.prepare(w, "xpbd_world_contact_report_counts"));
    for (int k = 0; k < 4; ++k)
        out[k] = w->report.counts[k];
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_download_pair_contacts(xpbd_world *w, xpbd_pair_contact *pairs, uint32_t pair_cap, xpbd_contact_point *points,
                                      uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points)
try {
    if (!w || !n_pairs || !n_points || (!pairs && pair_cap) || (!points && point_cap))
        return set_error(XPBD_E_INVALID, "xpbd_world_download_pair_contacts: NULL argument");
    XPBD_TRY(w->report.prepare(w, "xpbd_world_download_pair_contacts"));
    const uint32_t k = w->report.counts[0], total_points = w->report.counts[1];
    *n_pairs = k;
    *n_points = total_points;
    const uint32_t take = k < pair_cap ? k : pair_cap, take_points = points ? (total_points < point_cap ? total_points : point_cap) : 0u;
    if (take || take_points) {
        XPBD_HIP_TRY(w->report.pairs.reserve((size_t)k * sizeof(xpbd_pair_contact)));
        if (points)
            XPBD_HIP_TRY(w->report.points.reserve((size_t)at_least_one(total_points) * sizeof(xpbd_contact_point)));
        const uint32_t cur = w->report.cur;
        XPBD_HIP_TRY(xpbd::launch_report_records(w->report.frame_of(w->bp), w->report.keys[cur].as<unsigned long long>(), w->report.sel.as<uint32_t>(),
                                                 w->report.npts.as<uint32_t>(), k, w->report.pairs.as<xpbd_pair_contact>(),
                                                 points ? w->report.points.as<xpbd_contact_point>() : nullptr, w->stream));
        if (take)
            XPBD_HIP_TRY(hipMemcpyAsync(pairs, w->report.pairs.ptr, (size_t)take * sizeof(xpbd_pair_contact), hipMemcpyDeviceToHost, w->stream));
        if (take_points)
            XPBD_HIP_TRY(hipMemcpyAsync(points, w->report.points.ptr, (size_t)take_points * sizeof(xpbd_contact_point), hipMemcpyDeviceToHost,
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
    XPBD_TRY(w->report.prepare(w, "xpbd_world_download_contact_events"));
    const uint32_t total = w->report.counts[2] + w->report.counts[3];
    *n_out = total;
    const uint32_t take = total < cap ? total : cap;
    if (take) {
        const uint32_t cur = w->report.cur, k = w->report.counts[0], n_prev = w->report.prev_valid ? w->report.host[cur ^ 1u] : 0u;
        XPBD_HIP_TRY(w->report.events.reserve((size_t)total * sizeof(xpbd_contact_event)));
        XPBD_HIP_TRY(xpbd::launch_report_event_write(w->report.keys[cur].as<unsigned long long>(), k, w->report.keys[cur ^ 1u].as<unsigned long long>(),
                                                     n_prev, w->report.ev_flag.as<uint32_t>(), w->report.events.as<xpbd_contact_event>(), w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(out, w->report.events.ptr, (size_t)take * sizeof(xpbd_contact_event), hipMemcpyDeviceToHost, w->stream));
        XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_world_download_contact_events: %u events, capacity %u", total, cap);
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
    const ContactReport::ShardLoan loan(w->report, dev_owned, dev_global_id);
    uint32_t counts[4] = {0, 0, 0, 0}, n_pairs = 0, n_points = 0;
    int rc = xpbd_world_contact_report_counts(w, counts);
    if (rc == XPBD_OK) {
        pairs.resize(counts[0]);
        points.resize(counts[1]);
        rc = xpbd_world_download_pair_contacts(w, pairs.empty() ? nullptr : pairs.data(), counts[0], points.empty() ? nullptr : points.data(),
                                               counts[1], &n_pairs, &n_points);
    }
    return rc;
} catch (...) {
    return abi_exception("report_shard");
}
} // namespace xpbd
