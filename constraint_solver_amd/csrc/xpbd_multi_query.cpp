// xpbd_multi_query.cpp -- scene queries of the multi-GPU world (xpbd_multi.hpp): every local shard answers for its OWNED bodies,
// the answers of all ranks are gathered (with every rank's status) and merged by the rules of a single world (xpbd_merge.hpp).
#include <vector>

#include "xpbd_merge.hpp"
#include "xpbd_multi.hpp"

namespace xpbd::multi {
namespace {

// One shard's part of an overlap query: its OWNED bodies answer, under their global ids.  Counts first, then lists into a
// buffer of exactly that size; local_ids ascend, so every query's list is ascending in global index.
int shard_overlap(Shard &s, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, std::vector<uint32_t> &offsets,
                  std::vector<xpbd_overlap_hit> &hits)
{
    offsets.assign((size_t)n_queries + 1, 0);
    uint32_t total = 0;
    const int rc = xpbd::overlap_host(s.world, queries, n_queries, flags, offsets.data(), nullptr, 0, &total, s.query_ids.as<uint32_t>());
    if (rc != XPBD_OK && rc != XPBD_E_CAPACITY) // (a count of more than nothing comes back as "no room")
        return rc;
    hits.resize(total);
    if (total == 0)
        return XPBD_OK;
    return xpbd::overlap_host(s.world, queries, n_queries, flags, offsets.data(), hits.data(), total, &total, s.query_ids.as<uint32_t>());
}

// What the scene queries' argument checks (xpbd_checks.hpp) need to know of the world.
xpbd::QueryTarget query_target(const xpbd_multi_world *mw)
{
    return {mw->have_shapes, mw->plan.planned ? mw->n_global : 0u, (uint32_t)mw->shape_radius.size(), "xpbd_multi_world_set_polytopes"};
}

// The queries with one record per query (ray casts, sweeps, distances): every local shard answers for its owned bodies --
// per_shard(shard, its n records) -- then one all-gather of the hit records (with every rank's status) over all ranks, and every
// rank merges the n_ranks rows by the (distance, global index) rule of a single world (xpbd::merge_first_hits).
template <class Hit, class PerShard>
int gather_first_hits(xpbd_multi_world *mw, uint32_t n, Hit *hits, PerShard &&per_shard)
{
    LocalStatus st;
    std::vector<std::vector<Hit>> mine(mw->shards.size(), std::vector<Hit>(n));
    std::vector<const void *> send;
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        if (st.ok())
            st.keep(per_shard(mw->shards[k], mine[k].data()));
        send.push_back(mine[k].data());
    }
    std::vector<uint8_t> all;
    XPBD_TRY(all_gather_host(mw, send, (size_t)n * sizeof(Hit), all, st));
    xpbd::merge_first_hits(all.data(), mw->n_ranks, n, hits);
    return XPBD_OK;
}

// xpbd_multi_world_raycast(_masked), named `who` in its errors.
int multi_raycast(const char *who, xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, bool masked, uint32_t mask,
                  xpbd_ray_hit *hits)
{
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_raycast(who, query_target(mw), rays, n_rays, flags, hits, true));
    if (!mw->plan.planned) // (a plan over no bodies will do: every ray misses)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    if (n_rays == 0)
        return XPBD_OK;
    return gather_first_hits(mw, n_rays, hits, [&](Shard &s, xpbd_ray_hit *mine) {
        return xpbd::raycast_host(s.world, rays, n_rays, flags, mine, s.query_ids.as<uint32_t>(), masked, mask);
    });
}

// xpbd_multi_world_overlap: every local shard answers for its owned bodies; the counts, the offsets and the hits of every
// rank are gathered and merged per query (xpbd::merge_overlap_lists).
int multi_overlap(xpbd_multi_world *mw, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                  xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
{
    const char *who = "xpbd_multi_world_overlap";
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_overlap(who, query_target(mw), queries, n_queries, flags, offsets, hits, cap, n_out, true));
    if (n_queries == 0) {
        if (n_out)
            *n_out = 0;
        return XPBD_OK;
    }
    const size_t nl = mw->shards.size();
    LocalStatus st;
    std::vector<std::vector<uint32_t>> my_offsets(nl, std::vector<uint32_t>((size_t)n_queries + 1, 0));
    RankLists<xpbd_overlap_hit> lists(nl);
    for (size_t k = 0; k < nl; ++k)
        if (st.ok())
            st.keep(shard_overlap(mw->shards[k], queries, n_queries, flags, my_offsets[k], lists.local[k]));
    XPBD_TRY(gather_counts(mw, st, lists));
    std::vector<const void *> send(nl);
    for (size_t k = 0; k < nl; ++k)
        send[k] = my_offsets[k].data();
    std::vector<uint8_t> all_offsets;
    XPBD_TRY(all_gather_host(mw, send, ((size_t)n_queries + 1) * sizeof(uint32_t), all_offsets, st));
    XPBD_TRY(gather_rows(mw, st, lists));
    uint64_t total = 0;
    for (uint32_t t : lists.counts)
        total += t;
    if (total > 0xFFFFFFFFull)
        return set_error(XPBD_E_INVALID, "%s: %llu hits do not fit the 32-bit offsets", who, (unsigned long long)total);
    *n_out = xpbd::merge_overlap_lists(all_offsets.data(), lists.rows.data(), lists.widest, mw->n_ranks, n_queries, offsets, hits, cap);
    if (*n_out > cap)
        return set_error(XPBD_E_CAPACITY, "%s: %u hits but room for %u", who, *n_out, cap);
    return XPBD_OK;
}

// xpbd_multi_world_sweep.
int multi_sweep(xpbd_multi_world *mw, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
{
    const char *who = "xpbd_multi_world_sweep";
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_sweep(who, query_target(mw), sweeps, n_sweeps, flags, hits, true));
    if (n_sweeps == 0)
        return XPBD_OK;
    return gather_first_hits(mw, n_sweeps, hits, [&](Shard &s, xpbd_sweep_hit *mine) {
        return xpbd::sweep_host(s.world, sweeps, n_sweeps, flags, mine, s.query_ids.as<uint32_t>());
    });
}

// xpbd_multi_world_distance.
int multi_distance(xpbd_multi_world *mw, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits)
{
    const char *who = "xpbd_multi_world_distance";
    XPBD_TRY(check_usable(mw, who));
    XPBD_TRY(xpbd::check_distance(who, query_target(mw), queries, n_queries, flags, hits, true));
    if (n_queries == 0)
        return XPBD_OK;
    return gather_first_hits(mw, n_queries, hits, [&](Shard &s, xpbd_distance_hit *mine) {
        return xpbd::distance_host(s.world, queries, n_queries, flags, mine, s.query_ids.as<uint32_t>());
    });
}

} // namespace
} // namespace xpbd::multi

using namespace xpbd::multi;

extern "C" {

int xpbd_multi_world_raycast(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, xpbd_ray_hit *hits)
try {
    return multi_raycast("xpbd_multi_world_raycast", mw, rays, n_rays, flags, false, 0u, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_raycast_masked(xpbd_multi_world *mw, const xpbd_ray *rays, uint32_t n_rays, uint32_t flags, uint32_t mask,
                                    xpbd_ray_hit *hits)
try {
    return multi_raycast("xpbd_multi_world_raycast_masked", mw, rays, n_rays, flags, true, mask, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_overlap(xpbd_multi_world *mw, const xpbd_overlap_query *queries, uint32_t n_queries, uint32_t flags, uint32_t *offsets,
                             xpbd_overlap_hit *hits, uint32_t cap, uint32_t *n_out)
try {
    return multi_overlap(mw, queries, n_queries, flags, offsets, hits, cap, n_out);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_sweep(xpbd_multi_world *mw, const xpbd_sweep *sweeps, uint32_t n_sweeps, uint32_t flags, xpbd_sweep_hit *hits)
try {
    return multi_sweep(mw, sweeps, n_sweeps, flags, hits);
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_distance(xpbd_multi_world *mw, const xpbd_distance_query *queries, uint32_t n_queries, uint32_t flags, xpbd_distance_hit *hits)
try {
    return multi_distance(mw, queries, n_queries, flags, hits);
} XPBD_MULTI_ABI_CATCH

} // extern "C"
