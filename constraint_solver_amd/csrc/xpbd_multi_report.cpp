// xpbd_multi_report.cpp -- contact reports of the multi-GPU world (xpbd_multi.hpp): WorldReport's methods, one shard's part of a
// frame's report, the gather and merge at the end of an accepted frame (xpbd_merge.hpp), and the four report entry points.
#include <algorithm>
#include <cstring>
#include <vector>

#include "xpbd_merge.hpp"
#include "xpbd_multi.hpp"

namespace xpbd::multi {

void WorldReport::clear()
{
    valid = false;
    pairs.clear();
    points.clear();
    events.clear();
    prev.clear();
    begins = 0;
}

void WorldReport::enable(bool enable)
{
    clear();
    on = enable;
}

void WorldReport::accept(std::vector<xpbd_pair_contact> &merged, std::vector<xpbd_contact_point> &merged_points, std::vector<uint64_t> &keys)
{
    std::vector<xpbd_contact_event> new_events;
    begins = xpbd::contact_events(keys, prev, new_events);
    pairs.swap(merged);
    points.swap(merged_points);
    events.swap(new_events);
    prev.swap(keys);
    valid = true;
}

namespace {

// One shard's part of the frame's report: the pairs whose lower body it owns (the owner holds the other body as well, owned
// or as a ghost), under global ids.  local_ids are ascending, so the shard's list is sorted by global key.
int shard_report(Shard &s, std::vector<xpbd_pair_contact> &pairs, std::vector<xpbd_contact_point> &points)
{
    XPBD_TRY(bind(s));
    if (xpbd_world_body_count(s.world) != s.local_ids.size())
        return set_error(XPBD_E_INVALID, "contact report: shard %u holds %u bodies, its plan %zu", s.rank, xpbd_world_body_count(s.world),
                         s.local_ids.size());
    return xpbd::report_shard(s.world, s.report_owned.as<uint8_t>(), s.report_ids.as<uint32_t>(), pairs, points);
}

int check_report(const xpbd_multi_world *mw, const char *who)
{
    XPBD_TRY(check_usable(mw, who));
    if (!mw->report.on)
        return set_error(XPBD_E_INVALID, "%s: contact reports are off (xpbd_multi_world_set_contact_report)", who);
    if (!mw->report.valid)
        return set_error(XPBD_E_INVALID, "%s: no report: no frame has been stepped since the reports were enabled, the bodies uploaded "
                                         "or a step failed", who);
    return XPBD_OK;
}

} // namespace

// Collective, at the end of an accepted frame: every rank gathers every shard's list, merges them by key (the lists are
// disjoint: a pair belongs to the owner of its lower body) and derives the events from the merged lists, so that owners
// changing at a re-plan do not matter.  Same records as one world over the same bodies.
int capture_report(xpbd_multi_world *mw)
{
    const size_t nl = mw->shards.size();
    LocalStatus st;
    RankLists<xpbd_pair_contact> pairs(nl);
    RankLists<xpbd_contact_point> points(nl);
    for (size_t k = 0; k < nl; ++k)
        if (st.ok())
            st.keep(shard_report(mw->shards[k], pairs.local[k], points.local[k]));
    XPBD_TRY(gather_counts(mw, st, pairs, points));
    XPBD_TRY(gather_rows(mw, st, pairs));
    XPBD_TRY(gather_rows(mw, st, points));
    std::vector<xpbd_pair_contact> merged;
    std::vector<xpbd_contact_point> merged_points;
    std::vector<uint64_t> keys;
    xpbd::merge_contact_reports(pairs.rows.data(), pairs.widest, pairs.counts.data(), points.rows.data(), points.widest, mw->n_ranks, merged, merged_points, keys);
    mw->report.accept(merged, merged_points, keys);
    return XPBD_OK;
}

} // namespace xpbd::multi

using namespace xpbd::multi;

extern "C" {

int xpbd_multi_world_set_contact_report(xpbd_multi_world *mw, uint32_t enable)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_set_contact_report"));
    if (enable > 1u)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_set_contact_report: enable must be 0 or 1, not %u", enable);
    mw->report.enable(false);
    for (Shard &s : mw->shards) // the shards count their touching substeps; their lists are gathered by the step
        XPBD_TRY(xpbd_world_set_contact_report(s.world, enable));
    mw->report.enable(enable != 0);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_contact_report_counts(xpbd_multi_world *mw, uint32_t out[4])
try {
    if (mw && !out)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_contact_report_counts: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_contact_report_counts"));
    const WorldReport &r = mw->report;
    out[0] = (uint32_t)r.pairs.size();
    out[1] = (uint32_t)r.points.size();
    out[2] = r.begins;
    out[3] = (uint32_t)r.events.size() - r.begins;
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download_pair_contacts(xpbd_multi_world *mw, xpbd_pair_contact *pairs, uint32_t pair_cap, xpbd_contact_point *points,
                                            uint32_t point_cap, uint32_t *n_pairs, uint32_t *n_points)
try {
    if (mw && (!n_pairs || !n_points || (!pairs && pair_cap) || (!points && point_cap)))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_pair_contacts: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_download_pair_contacts"));
    const WorldReport &r = mw->report;
    const uint32_t k = (uint32_t)r.pairs.size(), total_points = (uint32_t)r.points.size();
    *n_pairs = k;
    *n_points = total_points;
    if (pair_cap)
        std::memcpy(pairs, r.pairs.data(), (size_t)std::min(k, pair_cap) * sizeof(xpbd_pair_contact));
    if (points && point_cap)
        std::memcpy(points, r.points.data(), (size_t)std::min(total_points, point_cap) * sizeof(xpbd_contact_point));
    if (k > pair_cap || (points && total_points > point_cap))
        return set_error(XPBD_E_CAPACITY, "xpbd_multi_world_download_pair_contacts: %u pairs, capacity %u; %u points, capacity %u", k, pair_cap,
                         total_points, point_cap);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_download_contact_events(xpbd_multi_world *mw, xpbd_contact_event *out, uint32_t cap, uint32_t *n_out)
try {
    if (mw && (!n_out || (!out && cap)))
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_download_contact_events: NULL argument");
    XPBD_TRY(check_report(mw, "xpbd_multi_world_download_contact_events"));
    const WorldReport &r = mw->report;
    const uint32_t total = (uint32_t)r.events.size();
    *n_out = total;
    if (cap)
        std::memcpy(out, r.events.data(), (size_t)std::min(total, cap) * sizeof(xpbd_contact_event));
    if (total > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_multi_world_download_contact_events: %u events, capacity %u", total, cap);
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

} // extern "C"
