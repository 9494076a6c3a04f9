// plan_standalone_main.cpp -- the shard planner (csrc/xpbd_plan.cpp + csrc/xpbd_error.cpp) on its own, with no device and no
// Python: built by tests/test_plan_standalone.py with plain g++, also under ASan/UBSan and TSan.  Exits non-zero with a
// one-line message on the first difference.  Same properties as tests/test_halo_plan_native.py, through the C ABI; then, through
// the C++ header, what a re-plan makes of the plans: full and light plan of every rank agree, and the layout of every shard
// (layout_shard: local slots, source map, ghost rows, joints) equals a brute-force reading of the same plans.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_plan.hpp"

namespace {

struct Lcg { // Knuth's MMIX constants; the high bits
    uint64_t state;
    uint32_t next() { return (uint32_t)((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
    double uniform() { return (double)next() / 2147483648.0; } // [0, 1)
};

struct Scene {
    const char *name;
    uint32_t n;
    double edge, extent[3]; // the bodies' centres: uniform in a box of this size
};

int fail(const Scene &s, uint32_t n_ranks, const char *what, uint32_t rank, uint32_t at)
{
    std::fprintf(stderr, "plan_standalone: %s, %u ranks: %s (rank %u, entry %u) -- %s\n", s.name, n_ranks, what, rank, at, xpbd_last_error());
    return 1;
}

using namespace xpbd::plan;

// The lists of all ranks as a collective gathers them: row r = rank r's list, padded to the longest with a pattern that is no id.
struct Gathered {
    std::vector<uint32_t> ids, counts;
    uint32_t width = 1;
    explicit Gathered(const std::vector<std::vector<uint32_t>> &lists)
    {
        for (const auto &l : lists)
            width = std::max(width, (uint32_t)l.size());
        ids.assign(lists.size() * width, 0xEEEEEEEEu);
        for (size_t r = 0; r < lists.size(); ++r) {
            counts.push_back((uint32_t)lists[r].size());
            std::copy(lists[r].begin(), lists[r].end(), ids.begin() + r * width);
        }
    }
    RankIds view() const { return RankIds{ids.data(), counts.data(), width, (uint32_t)counts.size()}; }
    void remove(uint32_t rank, uint32_t g) // takes g off the list of `rank`
    {
        uint32_t *lo = ids.data() + (size_t)rank * width, *hi = lo + counts[rank];
        std::copy(std::find(lo, hi, g) + 1, hi, std::find(lo, hi, g));
        hi[-1] = 0xEEEEEEEEu;
        --counts[rank];
    }
};

bool clean(const std::vector<int32_t> &slot_of) { return std::all_of(slot_of.begin(), slot_of.end(), [](int32_t v) { return v == -1; }); }

// layout_shard must refuse with XPBD_E_HIP and a message holding `text`, and leave the scratch as it found it.
bool refused(int rc, const char *text, const std::vector<int32_t> &slot_of)
{
    return rc == XPBD_E_HIP && std::strstr(xpbd_last_error(), text) && std::strstr(xpbd_last_error(), "(inconsistent plans)") && clean(slot_of);
}

// What a re-plan after the motion k0 -> k1 makes of every rank's shard: the moved pieces of xpbd_multi.cpp against brute force.
int run_layouts(const Scene &s, uint32_t w, const std::vector<int64_t> &k0, const std::vector<int64_t> &k1, const std::vector<xpbd_joint> &joints)
{
    const uint32_t n = s.n, n_joints = (uint32_t)joints.size();
    const double margin = 0.5;
    // 1. the owners from k0 give what every rank holds (at slots of its own choosing); the kept cuts give the owners after the motion
    std::vector<Cut> cuts;
    int axes[3];
    std::vector<uint8_t> holder(n), owner(n);
    compute_owners(k0.data(), n, w, holder.data(), cuts, axes);
    std::vector<std::vector<uint32_t>> held_ids(w), held_slots(w);
    std::vector<std::vector<int64_t>> held_keys(w), held_slab(w);
    std::vector<std::vector<uint8_t>> held_owner(w);
    uint32_t migrated = 0, cut_joints = 0, ghost_joints = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const uint32_t h = holder[g];
        const int64_t slab = slab_key(k1[g], axes);
        owner[g] = (uint8_t)owner_of(cuts, slab, g);
        migrated += owner[g] != h;
        held_slots[h].push_back(2 * (uint32_t)held_ids[h].size() + 1);
        held_ids[h].push_back(g);
        held_keys[h].push_back(k1[g]);
        held_slab[h].push_back(slab);
        held_owner[h].push_back(owner[g]);
    }
    for (const xpbd_joint &j : joints)
        cut_joints += owner[j.body_a] != owner[j.body_b];
    // 2. every rank's new plan from the global arrays; 3. the light plan from the rims gives the same, field by field
    JointLists joint_lists;
    joint_lists.build(joints.data(), n_joints, n);
    const JointIndex ji = joint_lists.view(joints.data());
    const std::vector<int64_t> cut_layers = cut_layers_of(cuts);
    std::vector<int32_t> slot_of(n, -1);
    KnownMap known;
    for (uint32_t h = 0; h < w; ++h) {
        std::vector<RimRow> rim;
        rim_rows_of(h, held_ids[h], held_keys[h], held_owner[h], held_slab[h], cut_layers, ji, slot_of, rim);
        for (const RimRow &r : rim)
            known.emplace(r.id, Known{r.key, r.owner, (uint8_t)h});
    }
    std::vector<ShardPlan> plans(w);
    std::vector<std::vector<uint32_t>> boundary_lists(w), export_lists(w);
    for (uint32_t r = 0; r < w; ++r) {
        ShardPlan &pl = plans[r], light;
        full_rank_plan(r, held_ids[r], k1.data(), owner.data(), holder.data(), n, joints.data(), n_joints, pl);
        if (light_rank_plan(r, held_ids[r], held_keys[r], held_owner[r], known, ji, slot_of, light))
            return fail(s, w, "light_rank_plan failed", r, 0);
        exports_of(r, held_ids[r], held_owner[r], light.boundary, light.exports);
        if (light.own != pl.own || light.own_holder != pl.own_holder || light.ghosts != pl.ghosts || light.ghost_owner != pl.ghost_owner ||
            light.ghost_holder != pl.ghost_holder || light.boundary != pl.boundary || light.far != pl.far || light.exports != pl.exports)
            return fail(s, w, "the light plan and the full plan of a rank differ in a field", r, 0);
        boundary_lists[r] = pl.boundary, export_lists[r] = pl.exports;
    }
    // 4. every shard's layout against brute force
    const Gathered boundary(boundary_lists), exports(export_lists);
    const uint32_t rows = boundary.width;
    const double edge = s.edge, near_scale = 1.0 / (margin * margin), far_scale = 1.0 / ((margin + 0.5 * edge) * (margin + 0.5 * edge));
    for (uint32_t r = 0; r < w; ++r) {
        const ShardPlan &pl = plans[r];
        ShardLayout lay;
        if (layout_shard(r, pl, held_ids[r], held_slots[r], boundary.view(), exports.view(), rows, ji, slot_of, margin, edge, lay))
            return fail(s, w, "layout_shard failed", r, 0);
        if (!clean(slot_of))
            return fail(s, w, "layout_shard left marks in slot_of", r, 0);
        // per body of the world: 0 elsewhere, 1 owned here, 2 a ghost here; its slot
        std::vector<uint8_t> here(n, 0);
        std::vector<uint32_t> slot(n, UINT32_MAX);
        for (uint32_t g : pl.own)
            here[g] = 1;
        for (uint32_t g : pl.ghosts)
            here[g] = here[g] ? 3 : 2;
        std::vector<uint32_t> want_ids;
        for (uint32_t g = 0; g < n; ++g)
            if (here[g]) {
                if (here[g] == 3)
                    return fail(s, w, "a body is both owned and a ghost", r, g);
                slot[g] = (uint32_t)want_ids.size();
                want_ids.push_back(g);
            }
        const size_t n_loc = want_ids.size();
        if (lay.local_ids != want_ids)
            return fail(s, w, "local_ids is not the ascending union of own and ghosts", r, 0);
        if (lay.owned_slots.size() != pl.own.size() || lay.ghost_slots.size() != pl.ghosts.size() || lay.ghost_rows.size() != pl.ghosts.size() ||
            lay.boundary_slots.size() != pl.boundary.size() || lay.src.size() != n_loc || lay.skip.size() != n_loc || lay.owned.size() != n_loc ||
            lay.query_ids.size() != n_loc || lay.disp_scale.size() != pl.own.size() || lay.joints.size() != lay.joint_ids.size())
            return fail(s, w, "a list of the layout has the wrong length", r, 0);
        for (size_t i = 0; i < pl.own.size(); ++i)
            if (lay.owned_slots[i] != slot[pl.own[i]] || lay.disp_scale[i] != (pl.far[i] ? far_scale : near_scale))
                return fail(s, w, "an owned body's slot or allowance scale is wrong", r, (uint32_t)i);
        std::vector<uint8_t> want_skip(n_loc, 0);
        for (size_t i = 0; i < pl.ghosts.size(); ++i) {
            const uint32_t g = pl.ghosts[i], o = owner[g];
            const auto &list = boundary_lists[o];
            const size_t at = (size_t)(std::find(list.begin(), list.end(), g) - list.begin());
            if (lay.ghost_slots[i] != slot[g] || at == list.size() || lay.ghost_rows[i] != o * rows + at)
                return fail(s, w, "a ghost's slot or its row in the all-gather is wrong", r, (uint32_t)i);
            want_skip[slot[g]] = 1;
        }
        for (size_t i = 0; i < pl.boundary.size(); ++i) {
            if (lay.boundary_slots[i] != slot[pl.boundary[i]])
                return fail(s, w, "a boundary body's slot is wrong", r, (uint32_t)i);
            want_skip[slot[pl.boundary[i]]] = 1;
        }
        if (lay.skip != want_skip)
            return fail(s, w, "skip is not boundary + ghosts", r, 0);
        uint32_t arrivals = 0;
        for (size_t q = 0; q < n_loc; ++q) {
            const uint32_t g = want_ids[q];
            if (lay.owned[q] != (here[g] == 1) || lay.query_ids[q] != (here[g] == 1 ? g : XPBD_NO_HIT))
                return fail(s, w, "the owned mask or the query ids are wrong", r, (uint32_t)q);
            const bool stays = here[g] == 1 && holder[g] == r;
            if (stays) {
                const size_t i = (size_t)(std::find(held_ids[r].begin(), held_ids[r].end(), g) - held_ids[r].begin());
                if (lay.src[q] < 0 || (uint32_t)lay.src[q] != held_slots[r][i])
                    return fail(s, w, "a body that stays does not come from its old slot", r, (uint32_t)q);
                continue;
            }
            if (lay.src[q] != -(int32_t)(++arrivals) || lay.incoming.size() < arrivals)
                return fail(s, w, "the arrivals are not numbered -1, -2, ... in slot order", r, (uint32_t)q);
            const ShardLayout::Incoming in = lay.incoming[arrivals - 1];
            if (in.holder != holder[g] || in.row >= export_lists[in.holder].size() || export_lists[in.holder][in.row] != g)
                return fail(s, w, "an arrival's record is not that body's in its holder's export list", r, (uint32_t)q);
        }
        if (lay.incoming.size() != arrivals)
            return fail(s, w, "more incoming records than arrivals", r, arrivals);
        std::vector<uint32_t> want_joints;
        for (uint32_t j = 0; j < n_joints; ++j)
            if (here[joints[j].body_a] && here[joints[j].body_b])
                want_joints.push_back(j);
        if (lay.joint_ids != want_joints)
            return fail(s, w, "joint_ids is not the joints with both ends here", r, 0);
        for (size_t q = 0; q < want_joints.size(); ++q) {
            const xpbd_joint &j = joints[want_joints[q]];
            xpbd_joint l = lay.joints[q];
            if (l.body_a != slot[j.body_a] || l.body_b != slot[j.body_b])
                return fail(s, w, "a local joint's ends are not the slots of its bodies", r, (uint32_t)q);
            l.body_a = j.body_a, l.body_b = j.body_b;
            if (std::memcmp(&l, &j, sizeof j) != 0)
                return fail(s, w, "a local joint differs from the global one in more than its ends", r, (uint32_t)q);
            ghost_joints += here[j.body_a] == 2 || here[j.body_b] == 2;
        }
        // joint records: the caller's order kept, joints outside the shard dropped, local joint numbers
        std::vector<xpbd_joint_limit> limits;
        for (uint32_t k = 0; k < 2 * n_joints; ++k) {
            xpbd_joint_limit l{};
            l.joint = (k * 7 + 3) % n_joints, l.kind = k, l.lower = -(double)k, l.upper = (double)k;
            limits.push_back(l);
        }
        const std::vector<xpbd_joint_limit> local = local_joint_records(limits, lay.joint_ids);
        size_t at = 0;
        for (const xpbd_joint_limit &l : limits) {
            const auto it = std::find(want_joints.begin(), want_joints.end(), l.joint);
            if (it == want_joints.end())
                continue;
            if (at == local.size() || local[at].joint != (uint32_t)(it - want_joints.begin()) || local[at].kind != l.kind || local[at].upper != l.upper)
                return fail(s, w, "a joint limit was not re-indexed in the caller's order", r, (uint32_t)at);
            ++at;
        }
        if (at != local.size())
            return fail(s, w, "more local joint limits than limits on the shard's joints", r, (uint32_t)at);
        for (uint32_t g : {0u, n / 2, n - 1})
            if (slot_in_shard(lay.local_ids, g) != (here[g] ? (int32_t)slot[g] : -1))
                return fail(s, w, "slot_in_shard is wrong", r, g);
        // plans that do not fit together are refused (the sanitizer builds: without a read out of bounds)
        if (!pl.ghosts.empty()) {
            Gathered broken = boundary;
            broken.remove(owner[pl.ghosts[0]], pl.ghosts[0]);
            if (!refused(layout_shard(r, pl, held_ids[r], held_slots[r], broken.view(), exports.view(), rows, ji, slot_of, margin, edge, lay),
                         "is mirrored by rank", slot_of))
                return fail(s, w, "a ghost missing from its owner's boundary list was not refused", r, pl.ghosts[0]);
        }
        for (size_t i = 0; i < pl.own.size(); ++i)
            if (pl.own_holder[i] != r) { // the first arrival
                Gathered broken = exports;
                broken.remove(pl.own_holder[i], pl.own[i]);
                if (!refused(layout_shard(r, pl, held_ids[r], held_slots[r], boundary.view(), broken.view(), rows, ji, slot_of, margin, edge, lay),
                             "is needed by rank", slot_of))
                    return fail(s, w, "an arrival missing from its holder's export list was not refused", r, pl.own[i]);
                ShardPlan claims = pl;
                claims.own_holder[i] = (uint8_t)r;
                if (!refused(layout_shard(r, claims, held_ids[r], held_slots[r], boundary.view(), exports.view(), rows, ji, slot_of, margin, edge, lay),
                             "is not among the bodies rank", slot_of))
                    return fail(s, w, "a body the rank claims to hold but does not was not refused", r, pl.own[i]);
                break;
            }
    }
    // a rank that is out of range, lists without entries: not found, nothing read
    if (boundary.view().find(w, 0) != -1 || RankIds{nullptr, std::vector<uint32_t>(w, 0).data(), 1, w}.find(0, 0) != -1)
        return fail(s, w, "RankIds::find found something in no list", 0, 0);
    if (migrated == 0 || cut_joints == 0 || ghost_joints == 0)
        return fail(s, w, "the scene lacks a body that changes owner, a joint across a cut or a joint with a ghost end on a shard", migrated, cut_joints);
    return 0;
}

int run(const Scene &s)
{
    const uint32_t n = s.n, n_joints = 40;
    Lcg rng{0x9E3779B97F4A7C15ull ^ n};
    // cell keys at the cut, and after every body has moved by less than one cell along every axis
    std::vector<int64_t> k0(n), k1(n);
    for (uint32_t g = 0; g < n; ++g) {
        double c0[3], c1[3];
        for (int a = 0; a < 3; ++a) {
            c0[a] = rng.uniform() * s.extent[a];
            c1[a] = c0[a] + (rng.uniform() - 0.5) * 1.96 * s.edge;
        }
        k0[g] = xpbd_halo_cell_key(c0, s.edge);
        k1[g] = xpbd_halo_cell_key(c1, s.edge);
    }
    std::vector<xpbd_joint> joints(n_joints, xpbd_joint{}); // random bodies up to 200 ids apart: many cross shard boundaries
    for (xpbd_joint &j : joints) {
        j.body_a = rng.next() % (n - 200);
        j.body_b = j.body_a + 1 + rng.next() % 199;
    }
    for (uint32_t w : {2u, 3u, 5u}) {
        // 1. ownership is a function of the keys alone
        std::vector<uint8_t> owner(n), again(n);
        if (xpbd_halo_partition(k0.data(), n, w, owner.data()) || xpbd_halo_partition(k0.data(), n, w, again.data()))
            return fail(s, w, "xpbd_halo_partition failed", 0, 0);
        for (uint32_t g = 0; g < n; ++g)
            if (owner[g] != again[g] || owner[g] >= w)
                return fail(s, w, "the owners of a second call differ", owner[g], g);
        // 2. a body is on its owner's boundary list iff another rank lists it as a ghost
        std::vector<uint8_t> on_boundary(n, 0), mirrored(n, 0), far(n);
        std::vector<uint32_t> ghosts(n), boundary(n);
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t n_ghosts = 0, n_boundary = 0;
            if (xpbd_halo_plan_owned(k0.data(), owner.data(), n, w, r, joints.data(), n_joints, ghosts.data(), &n_ghosts, boundary.data(), &n_boundary,
                                     nullptr, n))
                return fail(s, w, "xpbd_halo_plan_owned failed", r, 0);
            for (uint32_t i = 0; i < n_ghosts; ++i) {
                if (ghosts[i] >= n || owner[ghosts[i]] == r)
                    return fail(s, w, "a rank mirrors a body of its own", r, i);
                mirrored[ghosts[i]] = 1;
            }
            for (uint32_t i = 0; i < n_boundary; ++i) {
                if (boundary[i] >= n || owner[boundary[i]] != r)
                    return fail(s, w, "a boundary body is not the rank's", r, i);
                on_boundary[boundary[i]] = 1;
            }
        }
        for (uint32_t g = 0; g < n; ++g)
            if (on_boundary[g] != mirrored[g])
                return fail(s, w, "boundary lists and ghost lists disagree", owner[g], g);
        // 3. the light plan after the motion == the full planner with the owners the light plan reports
        std::vector<uint8_t> owner_now(n), far_light(n);
        std::vector<uint32_t> own(n), ghosts_light(n), boundary_light(n);
        for (uint32_t r = 0; r < w; ++r) {
            uint32_t n_own = 0, n_ghosts_light = 0, n_boundary_light = 0, n_ghosts = 0, n_boundary = 0;
            if (xpbd_halo_plan_light(k0.data(), k1.data(), n, w, r, joints.data(), n_joints, owner_now.data(), own.data(), &n_own, ghosts_light.data(),
                                     &n_ghosts_light, boundary_light.data(), &n_boundary_light, far_light.data(), n))
                return fail(s, w, "xpbd_halo_plan_light failed", r, 0);
            if (xpbd_halo_plan_owned(k1.data(), owner_now.data(), n, w, r, joints.data(), n_joints, ghosts.data(), &n_ghosts, boundary.data(), &n_boundary,
                                     far.data(), n))
                return fail(s, w, "xpbd_halo_plan_owned failed after the motion", r, 0);
            uint32_t k = 0;
            for (uint32_t g = 0; g < n; ++g)
                if (owner_now[g] == r && (k >= n_own || own[k++] != g))
                    return fail(s, w, "light plan: `own` is not the bodies the rank owns now", r, g);
            if (k != n_own || n_ghosts_light != n_ghosts || n_boundary_light != n_boundary)
                return fail(s, w, "light plan: list lengths differ from the full planner's", r, n_own);
            for (uint32_t i = 0; i < n_ghosts; ++i)
                if (ghosts_light[i] != ghosts[i])
                    return fail(s, w, "light plan: ghosts differ", r, i);
            for (uint32_t i = 0; i < n_boundary; ++i)
                if (boundary_light[i] != boundary[i])
                    return fail(s, w, "light plan: boundary differs", r, i);
            for (uint32_t i = 0; i < n_own; ++i)
                if (far_light[i] != far[i])
                    return fail(s, w, "light plan: far flags differ", r, i);
        }
        // 4. the layouts of the shards after that motion (the slab exists for the threaded passes)
        if (n < 65536)
            if (int rc = run_layouts(s, w, k0, k1, joints))
                return rc;
    }
    return 0;
}

} // namespace

int main()
{
    const double edge = 2.04;
    // 70 001: past the 65 536 bodies above which the planner's passes run in threads, in uneven chunks
    const Scene scenes[] = {{"cloud of 997", 997, edge, {12.0, 12.0, 12.0}}, {"slab of 70001", 70001, edge, {64 * edge, 8 * edge, 8 * edge}}};
    for (const Scene &s : scenes)
        if (int rc = run(s))
            return rc;
    std::puts("plan_standalone: ok");
    return 0;
}
