// xpbd_multi_plan.cpp -- a plan of the multi-GPU world (xpbd_multi.hpp): the plan-time collectives around the planner of
// xpbd_plan.hpp (cell keys or rims, boundary lists, the records of migrating and boundary bodies), the device half of a plan
// (re-pack, uploads), PlanState's methods, the owned bodies' state for a download, and xpbd_multi_world_replan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xpbd_multi.hpp"

namespace xpbd::multi {

void PlanState::reset_for_upload()
{
    planned = false;
    cuts_valid = false; // the first plan is a full one
    check_plans = std::getenv("XPBD_MULTI_CHECK_PLANS") != nullptr;
    plans = 0;
    full_plans = light_plans = 0;
}

void PlanState::accept(uint32_t rows, double edge)
{
    capacity = rows;
    cell_edge = edge;
    planned = true;
    violated = false;
    last_displacement = 0.0;
    ++plans;
}

void PlanState::accept_full(std::vector<uint8_t> &new_owner, std::vector<uint32_t> &new_count)
{
    owner.swap(new_owner);
    owned_count.swap(new_count);
    cuts_valid = true;
    balance_most = 0, balance_least = UINT32_MAX;
    for (uint32_t c : owned_count) {
        balance_most = std::max(balance_most, c);
        balance_least = std::min(balance_least, c);
    }
    ++full_plans;
}

void PlanState::accept_light(std::vector<uint32_t> &new_count)
{
    owner.clear(); // (rebuilt on demand: xpbd_multi_world_owners)
    owned_count.swap(new_count);
    ++light_plans;
}

namespace {

struct KeyRow {
    int64_t key;
    uint32_t id, unused;
};

// The cell keys of the bodies every local shard holds, computed where the bodies are (8 bytes per body come back).
int held_cell_keys(xpbd_multi_world *mw, LocalStatus &st, double edge, std::vector<std::vector<int64_t>> &held_keys)
{
    held_keys.assign(mw->shards.size(), std::vector<int64_t>());
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        Shard &s = mw->shards[k];
        const uint32_t cnt = (uint32_t)s.held_ids.size();
        held_keys[k].assign(cnt, 0);
        uint32_t bad = UINT32_MAX;
        if (st.ok())
            st.keep(xpbd::halo_cell_keys(s.world, s.owned_slots.as<uint32_t>(), cnt, edge, held_keys[k].data(), &bad));
        if (st.ok() && bad != UINT32_MAX)
            st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u has a non-finite position: it cannot be placed in the grid the shards "
                                              "are cut from", s.held_ids[bad]));
    }
    return XPBD_OK;
}

// One all-gather of 16 bytes per body: the cell key of every body of the world and who holds it.
int gather_world_keys(xpbd_multi_world *mw, LocalStatus &st, const std::vector<std::vector<int64_t>> &held_keys, uint64_t max_held,
                      std::vector<int64_t> &keys, std::vector<uint8_t> &holder)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    std::vector<std::vector<KeyRow>> key_rows(n_local);
    std::vector<const void *> send(n_local);
    std::vector<uint8_t> gathered;
    for (size_t k = 0; k < n_local; ++k) {
        const Shard &s = mw->shards[k];
        key_rows[k].assign(max_held, KeyRow{0, UINT32_MAX, 0});
        for (size_t i = 0; i < s.held_ids.size() && st.ok(); ++i)
            key_rows[k][i] = KeyRow{held_keys[k][i], s.held_ids[i], 0};
        send[k] = key_rows[k].data();
    }
    XPBD_TRY(all_gather_host(mw, send, (size_t)max_held * sizeof(KeyRow), gathered, st));
    keys.assign(n, 0);
    holder.assign(n, 0xFF);
    for (uint32_t r = 0; r < w && st.ok(); ++r) {
        const KeyRow *rows = reinterpret_cast<const KeyRow *>(gathered.data() + (size_t)r * max_held * sizeof(KeyRow));
        for (uint64_t i = 0; i < max_held; ++i) {
            if (rows[i].id == UINT32_MAX)
                break;
            if (rows[i].id >= n || holder[rows[i].id] != 0xFF) {
                st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u is held twice or out of range (rank %u)", rows[i].id, r));
                break;
            }
            keys[rows[i].id] = rows[i].key;
            holder[rows[i].id] = (uint8_t)r;
        }
    }
    return XPBD_OK;
}

// The second half of every plan: the boundary lists of all ranks fix the rows of the per-substep all-gather, the records of
// the bodies that change hands or are mirrored travel, and every shard's local world is re-packed on its device.  Collective.
int finish_plan(xpbd_multi_world *mw, LocalStatus &st, std::vector<ShardPlan> &plans, double edge, PlanTrace &trace)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    // 4. the boundary lists of all ranks (ascending global ids) fix the rows of the per-substep all-gather; the export lists
    //    those of the plan-time record exchange
    RankLists<uint32_t> boundary(n_local), exports(n_local);
    RankLists<BodyRecord> records(n_local);
    for (size_t k = 0; k < n_local && st.ok(); ++k)
        boundary.local[k] = plans[k].boundary, exports.local[k] = plans[k].exports;
    XPBD_TRY(gather_counts(mw, st, boundary, exports));
    XPBD_TRY(gather_rows(mw, st, boundary));
    // the records of the exported bodies: gathered on the device that holds them, 39 doubles each (nothing to exchange if
    // nobody exports anything: every rank sees that in the gathered counts)
    if (std::any_of(exports.counts.begin(), exports.counts.end(), [](uint32_t c) { return c > 0; })) {
        XPBD_TRY(gather_rows(mw, st, exports));
        records.counts = exports.counts, records.widest = exports.widest;
        std::vector<uint32_t> slots;
        for (size_t k = 0; k < n_local; ++k) {
            Shard &s = mw->shards[k];
            records.local[k].resize(records.widest);
            slots.clear();
            if (st.ok())
                for (uint32_t g : plans[k].exports)
                    slots.push_back(s.owned_slots_h[std::lower_bound(s.held_ids.begin(), s.held_ids.end(), g) - s.held_ids.begin()]);
            if (st.ok())
                st.keep(xpbd::download_records(s.world, slots.data(), (uint32_t)slots.size(), records.local[k][0].v));
        }
        XPBD_TRY(gather_rows(mw, st, records));
    }
    trace.lap("lists, exported records");

    // 5. every shard's local world: owned + ghost bodies in ascending global id (layout_shard), re-packed on its device
    const uint32_t rows = boundary.widest; // (rows per rank of the per-substep all-gather from now on: PlanState::capacity, set when the plan has succeeded)
    const RankIds boundary_ids{reinterpret_cast<const uint32_t *>(boundary.rows.data()), boundary.counts.data(), boundary.widest, w};
    const RankIds export_ids{reinterpret_cast<const uint32_t *>(exports.rows.data()), exports.counts.data(), exports.widest, w};
    const JointIndex ji = mw->settings.joint_lists.view(mw->settings.joints.data());
    std::vector<int32_t> &slot_of = mw->plan.slot_of;
    if (slot_of.size() != n)
        slot_of.assign(n, -1);
    auto build_shard = [&](size_t k) -> int {
        Shard &s = mw->shards[k];
        ShardPlan &pl = plans[k];
        XPBD_TRY(bind(s));
        ShardLayout lay;
        XPBD_TRY(layout_shard(s.rank, pl, s.held_ids, s.owned_slots_h, boundary_ids, export_ids, rows, ji, slot_of, mw->margin, edge, lay));
        std::vector<BodyRecord> incoming(lay.incoming.size());
        for (size_t i = 0; i < incoming.size(); ++i)
            incoming[i] = records.at(lay.incoming[i].holder, lay.incoming[i].row);
        const uint32_t n_own = (uint32_t)pl.own.size(), n_loc = (uint32_t)lay.local_ids.size();
        trace.lap("  source map of a shard");
        if (int rc = xpbd::repack_bodies(s.world, lay.src.data(), n_loc, incoming.empty() ? nullptr : incoming[0].v, (uint32_t)incoming.size()))
            return rc;
        trace.lap("  re-pack on the device");
        if (int rc = xpbd_world_set_joints(s.world, lay.joints.data(), (uint32_t)lay.joints.size()))
            return rc;
        s.joint_ids.swap(lay.joint_ids);
        XPBD_TRY(push_body_settings(mw, s, lay.local_ids));
        XPBD_HIP_TRY(hipStreamSynchronize(s.stream));
        trace.lap("  joints");
        XPBD_TRY(upload_vector(s.boundary_slots, lay.boundary_slots, s.stream));
        XPBD_TRY(upload_vector(s.ghost_slots, lay.ghost_slots, s.stream));
        XPBD_TRY(upload_vector(s.ghost_rows, lay.ghost_rows, s.stream));
        XPBD_TRY(upload_vector(s.owned_slots, lay.owned_slots, s.stream));
        XPBD_TRY(upload_vector(s.skip_flags, lay.skip, s.stream));
        XPBD_TRY(upload_vector(s.disp_scale, lay.disp_scale, s.stream));
        XPBD_TRY(upload_vector(s.query_ids, lay.query_ids, s.stream));
        XPBD_TRY(upload_vector(s.report_ids, lay.local_ids, s.stream));
        XPBD_TRY(upload_vector(s.report_owned, lay.owned, s.stream));
        XPBD_HIP_TRY(s.send.reserve((size_t)rows * kDyn * 8));
        XPBD_HIP_TRY(s.recv.reserve((size_t)w * rows * kDyn * 8));
        XPBD_HIP_TRY(hipMemsetAsync(s.send.ptr, 0, (size_t)rows * kDyn * 8, s.stream));
        XPBD_HIP_TRY(s.snapshot.reserve(std::max<size_t>((size_t)3 * n_own * 8, 8)));
        XPBD_HIP_TRY(s.disp.reserve(16));
        XPBD_HIP_TRY(s.disp_all.reserve((size_t)w * 16));
        if (int rc = xpbd_world_snapshot_positions(s.world, s.owned_slots.as<uint32_t>(), n_own, s.snapshot.as<double>()))
            return rc;
        XPBD_HIP_TRY(hipStreamSynchronize(s.stream)); // the layout's host vectors go out of scope
        s.owned_slots_h.swap(lay.owned_slots);
        s.local_ids.swap(lay.local_ids);
        s.held_ids.swap(pl.own); // from now on the shard holds what it owns
        s.ghosts.swap(pl.ghosts);
        s.boundary.swap(pl.boundary);
        s.far.swap(pl.far);
        trace.lap("  index lists of a shard");
        return XPBD_OK;
    };
    for (size_t k = 0; k < n_local && st.ok(); ++k) {
        st.keep(build_shard(k));
        if (!st.ok())
            mw->plan.tear(); // some shards re-packed, this one half-way: there is no plan to go back to (see make_plan)
    }
    // all ranks leave the plan together: a last status-only exchange (a failed re-pack on one rank fails the plan everywhere)
    std::vector<uint8_t> gathered;
    if (int rc = all_gather_host(mw, std::vector<const void *>(n_local, nullptr), 0, gathered, st)) {
        mw->plan.tear(); // (a shard of some rank failed while being re-packed)
        return rc;
    }
    mw->plan.accept(rows, edge);
    return XPBD_OK;
}

double plan_cell_edge(const xpbd_multi_world *mw, double rmax) { return 2.0 * (rmax + mw->pad + mw->margin); }

// (rmax of the world, bodies held per rank): the first collective of every plan
int gather_heads(xpbd_multi_world *mw, LocalStatus &st, double &rmax, uint64_t &max_held)
{
    struct Head {
        double rmax;
        uint64_t count;
    };
    const size_t n_local = mw->shards.size();
    std::vector<Head> head(n_local);
    std::vector<const void *> send(n_local);
    std::vector<uint8_t> gathered;
    for (size_t k = 0; k < n_local; ++k) {
        head[k] = Head{mw->rmax_local, mw->shards[k].held_ids.size()};
        send[k] = &head[k];
    }
    XPBD_TRY(all_gather_host(mw, send, sizeof(Head), gathered, st));
    rmax = 0.0, max_held = 0;
    uint64_t total_held = 0;
    for (uint32_t r = 0; r < mw->n_ranks; ++r) {
        Head h;
        std::memcpy(&h, gathered.data() + (size_t)r * sizeof(Head), sizeof h);
        rmax = std::max(rmax, h.rmax);
        max_held = std::max(max_held, h.count);
        total_held += h.count;
    }
    const double edge = plan_cell_edge(mw, rmax);
    if (!(edge > 0.0) || !(edge <= 1.0e300))
        st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: cell edge %g from radius %g, pad %g, halo_margin %g", edge, rmax, mw->pad, mw->margin));
    if (total_held != mw->n_global)
        st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: the ranks hold %llu bodies together, the world has %u", (unsigned long long)total_held,
                          mw->n_global));
    return XPBD_OK;
}

// A FULL plan: ownership re-cut from the cell keys of the whole world (every rank passes over 16 bytes per body of it), halos
// from the global keys and owners.  The first plan, and whenever the sticky cuts of the light plans have drifted out of balance.
// The bodies stay on the device: what crosses the bus is 8 bytes of cell key per owned body, the records of the bodies that
// change hands or are mirrored (a few per cent) and the index lists of the new plan.  Collective.  Local failures are
// carried through the collectives (LocalStatus: `st` may already hold one), so all ranks fail together.
int make_plan_full(xpbd_multi_world *mw, LocalStatus &st, PlanTrace &trace)
{
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    PlanState &ps = mw->plan;
    // 1. the largest bounding radius of the whole world (r_shape + |centroid - com|: conservative whatever the rotation;
    //    a property of the bodies, known since the upload) and how many bodies every rank owns
    double rmax = 0.0;
    uint64_t max_held = 0;
    XPBD_TRY(gather_heads(mw, st, rmax, max_held));
    const double edge = plan_cell_edge(mw, rmax);
    // 2. grid cell of every body of the world (centre = position + center_of_mass)
    std::vector<std::vector<int64_t>> held_keys;
    XPBD_TRY(held_cell_keys(mw, st, edge, held_keys));
    trace.lap("cell keys (device)");
    std::vector<int64_t> keys;
    std::vector<uint8_t> holder;
    XPBD_TRY(gather_world_keys(mw, st, held_keys, max_held, keys, holder));
    trace.lap("keys of the world");

    // 3. ownership: the cell sequence (longest axis first) cut into runs of near-equal body count; then who mirrors whom
    std::vector<uint8_t> owner(n, 0);
    std::vector<uint32_t> owned_count(w, 0);
    std::vector<ShardPlan> plans(n_local);
    uint64_t migrated = 0;
    if (st.ok()) {
        compute_owners(keys.data(), n, w, owner.data(), ps.cuts, ps.cut_axes);
        for (uint32_t g = 0; g < n; ++g) {
            ++owned_count[owner[g]];
            migrated += owner[g] != holder[g];
        }
        trace.lap("cuts, owners");
        for (size_t k = 0; k < n_local; ++k)
            full_rank_plan(mw->shards[k].rank, mw->shards[k].held_ids, keys.data(), owner.data(), holder.data(), n, mw->settings.joints.data(),
                           (uint32_t)mw->settings.joints.size(), plans[k]);
    }
    trace.lap("halo plans");
    XPBD_TRY(finish_plan(mw, st, plans, edge, trace));
    ps.accept_full(owner, owned_count);
    mw->timers.migrated = migrated;
    return XPBD_OK;
}

// A LIGHT plan: the cuts stay where the last full plan put them, so a body's owner follows from its own cell key, and what a
// rank must know of the others is the RIM -- the bodies within two layers of a cut (nobody else can lie within two cells of a
// foreign cell), the bodies that change owner, and the ends of joints that leave their holder.  Host work and traffic are
// proportional to the rank's own bodies plus the rims, not to the world.  Falls back to a full plan (same collectives on
// every rank: the decision is taken from gathered data) when the shards have drifted out of balance.
int make_plan_light(xpbd_multi_world *mw, LocalStatus &st, PlanTrace &trace, bool &done)
{
    done = false;
    const uint32_t n = mw->n_global, w = mw->n_ranks;
    const size_t n_local = mw->shards.size();
    PlanState &ps = mw->plan;
    std::vector<uint8_t> gathered;
    std::vector<const void *> send(n_local);
    double rmax = 0.0;
    uint64_t max_held = 0;
    XPBD_TRY(gather_heads(mw, st, rmax, max_held));
    const double edge = plan_cell_edge(mw, rmax);
    std::vector<std::vector<int64_t>> held_keys;
    XPBD_TRY(held_cell_keys(mw, st, edge, held_keys));
    trace.lap("cell keys (device)");
    // the new owner of every held body from the sticky cuts; how many bodies every rank sends to every rank
    std::vector<std::vector<uint8_t>> held_owner(n_local);
    std::vector<std::vector<int64_t>> held_slab(n_local);
    std::vector<std::vector<uint32_t>> tally(n_local, std::vector<uint32_t>(w, 0));
    for (size_t k = 0; k < n_local; ++k) {
        const Shard &s = mw->shards[k];
        held_owner[k].assign(s.held_ids.size(), (uint8_t)s.rank);
        held_slab[k].assign(s.held_ids.size(), 0);
        for (size_t i = 0; i < s.held_ids.size() && st.ok(); ++i) {
            held_slab[k][i] = slab_key(held_keys[k][i], ps.cut_axes);
            held_owner[k][i] = (uint8_t)owner_of(ps.cuts, held_slab[k][i], s.held_ids[i]);
            ++tally[k][held_owner[k][i]];
        }
        send[k] = tally[k].data();
    }
    XPBD_TRY(all_gather_host(mw, send, (size_t)w * 4, gathered, st));
    std::vector<uint32_t> owned_count(w, 0);
    uint64_t migrated = 0;
    for (uint32_t h = 0; h < w; ++h)
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t c;
            std::memcpy(&c, gathered.data() + ((size_t)h * w + r) * 4, 4);
            owned_count[r] += c;
            if (h != r)
                migrated += c;
        }
    {
        // out of balance (a tenth of a share off): time for new cuts
        const uint32_t share = std::max(1u, n / w);
        uint32_t most = 0, least = UINT32_MAX;
        for (uint32_t c : owned_count) {
            most = std::max(most, c);
            least = std::min(least, c);
        }
        // (against what the last full plan achieved: cuts snap to cell boundaries, a world of few cells is never even)
        if (most > ps.balance_most + share / 10 + 8 || least + share / 10 + 8 < ps.balance_least)
            return XPBD_OK; // (done stays false: the caller makes a full plan; every rank decides alike)
    }
    trace.lap("owners from the cuts");
    // the rims: (key, id, new owner) of the held bodies near a cut, changing owner, or at the end of a joint that leaves the shard
    const std::vector<int64_t> cut_layers = cut_layers_of(ps.cuts);
    const JointIndex ji = mw->settings.joint_lists.view(mw->settings.joints.data());
    RankLists<RimRow> rim(n_local);
    if (ps.slot_of.size() != n)
        ps.slot_of.assign(n, -1);
    for (size_t k = 0; k < n_local && st.ok(); ++k)
        rim_rows_of(mw->shards[k].rank, mw->shards[k].held_ids, held_keys[k], held_owner[k], held_slab[k], cut_layers, ji, ps.slot_of, rim.local[k]);
    XPBD_TRY(gather_counts(mw, st, rim));
    XPBD_TRY(gather_rows(mw, st, rim));
    if (trace.on)
        std::fprintf(stderr, "[xpbd plan %llu] rim rows per rank: up to %u\n", (unsigned long long)ps.plans, rim.widest);
    trace.lap("rims of the world");
    // everybody's rim by body id: (key, owner, holder)
    KnownMap known;
    if (st.ok()) {
        size_t total = 0;
        for (uint32_t c : rim.counts)
            total += c;
        known.reserve(total * 2 + 16);
        for (uint32_t h = 0; h < w && st.ok(); ++h) {
            for (uint32_t i = 0; i < rim.counts[h]; ++i) {
                const RimRow row = rim.at(h, i);
                if (row.id >= n || row.owner >= w || !known.emplace(row.id, Known{row.key, row.owner, (uint8_t)h}).second) {
                    st.keep(set_error(XPBD_E_INVALID, "xpbd_multi_world: body %u is held twice or out of range (rank %u)", row.id, h));
                    break;
                }
            }
        }
    }
    std::vector<ShardPlan> plans(n_local);
    for (size_t k = 0; k < n_local && st.ok(); ++k) {
        Shard &s = mw->shards[k];
        ShardPlan &pl = plans[k];
        st.keep(light_rank_plan(s.rank, s.held_ids, held_keys[k], held_owner[k], known, ji, ps.slot_of, pl));
        if (!st.ok())
            break;
        if (pl.own.size() != owned_count[s.rank]) {
            st.keep(set_error(XPBD_E_HIP, "xpbd_multi_world: rank %u is to own %u bodies but finds %zu (inconsistent plans)", s.rank, owned_count[s.rank],
                              pl.own.size()));
            break;
        }
        exports_of(s.rank, s.held_ids, held_owner[k], pl.boundary, pl.exports);
    }
    trace.lap("halo plans (light)");
    if (ps.check_plans) { // XPBD_MULTI_CHECK_PLANS=1: the same lists from the keys of the whole world (the full planner, same cuts)
        std::vector<int64_t> keys;
        std::vector<uint8_t> holder;
        XPBD_TRY(gather_world_keys(mw, st, held_keys, max_held, keys, holder));
        if (st.ok()) {
            std::vector<uint8_t> owner(n);
            for (uint32_t g = 0; g < n; ++g)
                owner[g] = (uint8_t)owner_of(ps.cuts, slab_key(keys[g], ps.cut_axes), g);
            for (size_t k = 0; k < n_local && st.ok(); ++k) {
                std::vector<uint32_t> own, ghosts, boundary;
                std::vector<uint8_t> far;
                HaloPlanner::plan_rank(keys.data(), owner.data(), n, mw->shards[k].rank, mw->settings.joints.data(), (uint32_t)mw->settings.joints.size(), own, ghosts, boundary, &far);
                const ShardPlan &pl = plans[k];
                if (own != pl.own || ghosts != pl.ghosts || boundary != pl.boundary || far != pl.far)
                    st.keep(set_error(XPBD_E_HIP, "xpbd_multi_world: the light plan of rank %u differs from the full planner's (own %zu / %zu, ghosts %zu / %zu, "
                                                  "boundary %zu / %zu)", mw->shards[k].rank, pl.own.size(), own.size(), pl.ghosts.size(), ghosts.size(),
                                      pl.boundary.size(), boundary.size()));
            }
        }
        trace.lap("checked against the full planner");
    }
    XPBD_TRY(finish_plan(mw, st, plans, edge, trace));
    ps.accept_light(owned_count);
    mw->timers.migrated = migrated;
    done = true;
    return XPBD_OK;
}

} // namespace

// Builds ownership and halos from the bodies the shards own AT THE MOMENT (the first time: the index slices the caller handed
// over, uploaded as they are) and re-packs every shard's local world.  Collective.
int make_plan(xpbd_multi_world *mw, LocalStatus &st)
{
    const uint64_t t_plan = now_ns();
    PlanTrace trace(mw->plan.plans);
    bool done = false;
    int rc = XPBD_OK;
    if (mw->plan.cuts_valid && mw->n_ranks > 1 && !(mw->flags & XPBD_MULTI_FULL_PLANS))
        rc = make_plan_light(mw, st, trace, done);
    if (rc == XPBD_OK && !done)
        rc = make_plan_full(mw, st, trace);
    mw->timers.ns_plan += now_ns() - t_plan;
    if (rc != XPBD_OK && mw->plan.plan_torn && !mw->broken) {
        // A plan that fails BEFORE any shard is re-packed leaves the old plan and the state as they were (every rank returns
        // the error); one that fails in the middle of the re-packing does not: the world cannot be used any more.
        return shards_disagree(mw, rc, nullptr);
    }
    return rc;
}

// The owned bodies' current state (ascending global id, like Shard::held_ids), for a download.
int fetch_owned(xpbd_multi_world *mw, std::vector<std::vector<double>> &held)
{
    held.assign(mw->shards.size(), std::vector<double>());
    for (size_t k = 0; k < mw->shards.size(); ++k) {
        Shard &s = mw->shards[k];
        XPBD_TRY(bind(s));
        const uint32_t n_loc = (uint32_t)s.local_ids.size();
        std::vector<double> aos((size_t)n_loc * kRigid);
        if (int rc = xpbd_world_download_bodies(s.world, reinterpret_cast<xpbd_rigid *>(aos.data()), n_loc))
            return rc;
        held[k].resize(s.held_ids.size() * kRigid);
        for (size_t i = 0; i < s.held_ids.size(); ++i)
            std::memcpy(&held[k][i * kRigid], &aos[(size_t)s.owned_slots_h[i] * kRigid], kRigid * 8);
    }
    return XPBD_OK;
}

int replan(xpbd_multi_world *mw)
{
    LocalStatus st;
    return make_plan(mw, st);
}

} // namespace xpbd::multi

using namespace xpbd::multi;

extern "C" {

int xpbd_multi_world_replan(xpbd_multi_world *mw)
try {
    XPBD_TRY(check_usable(mw, "xpbd_multi_world_replan"));
    if (!mw->plan.planned)
        return set_error(XPBD_E_INVALID, "xpbd_multi_world_replan: no bodies uploaded");
    return replan(mw);
} XPBD_MULTI_ABI_CATCH

} // extern "C"
