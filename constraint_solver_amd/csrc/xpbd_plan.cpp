// xpbd_plan.cpp -- the shard planner (xpbd_plan.hpp) and the host-only diagnostics xpbd_halo_* of include/xpbd.h.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <thread>
#include <unordered_set>

#include "xpbd_error.h"
#include "xpbd_plan.hpp"

namespace xpbd {
namespace plan {
namespace {

int64_t clamp_cell(double q)
{
    const double lim = (double)kCellLimit;
    if (!(q >= -lim)) // NaN or far negative
        return -kCellLimit;
    return q > lim ? kCellLimit : (int64_t)q;
}

// The planner's passes over ALL bodies of the world (every rank makes them at every re-plan) in a few host threads.
// fn(thread, begin, end) for contiguous chunks in thread order; small inputs stay on the calling thread.
constexpr unsigned kPlanThreads = 8;

unsigned plan_threads(size_t n)
{
    static const unsigned hw = [] { // XPBD_PLAN_THREADS=<1..8> overrides (1: everything on the calling thread)
        const char *e = std::getenv("XPBD_PLAN_THREADS");
        const unsigned want = e ? (unsigned)std::atoi(e) : std::thread::hardware_concurrency();
        return std::max(1u, std::min(kPlanThreads, want));
    }();
    return n < ((size_t)1 << 16) ? 1u : hw;
}

// An exception in any chunk, or a thread that cannot be started, is rethrown on the calling thread (the first in thread order)
// once every thread that did start has been joined.
template <class F>
void parallel_chunks(size_t n, F fn)
{
    const unsigned t_count = plan_threads(n);
    if (t_count == 1) {
        fn(0u, (size_t)0, n);
        return;
    }
    std::exception_ptr error[kPlanThreads];
    auto chunk = [&](unsigned t) {
        try {
            fn(t, n * t / t_count, n * (t + 1) / t_count);
        } catch (...) {
            error[t] = std::current_exception();
        }
    };
    std::vector<std::thread> threads;
    threads.reserve(t_count - 1);
    try {
        for (unsigned t = 1; t < t_count; ++t)
            threads.emplace_back(chunk, t);
        chunk(0);
    } catch (...) {
        error[0] = std::current_exception();
    }
    for (std::thread &th : threads)
        th.join();
    for (const std::exception_ptr &e : error)
        if (e)
            std::rethrow_exception(e);
}

// A box of cells: what a pass over bodies reduces to (one per thread, merged in thread order).
struct CellBox {
    int64_t lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    void add(int64_t key)
    {
        int64_t c[3];
        cell_of_key(key, c);
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], c[a]);
            hi[a] = std::max(hi[a], c[a]);
        }
    }
    void merge(const CellBox &o)
    {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], o.lo[a]);
            hi[a] = std::max(hi[a], o.hi[a]);
        }
    }
};

// The box of the cells of keys[0 .. n), in a few threads.
CellBox box_of_keys(const int64_t *keys, size_t n)
{
    CellBox part[kPlanThreads], box;
    parallel_chunks(n, [&](unsigned t, size_t begin, size_t end) {
        CellBox mine;
        for (size_t g = begin; g < end; ++g)
            mine.add(keys[g]);
        part[t] = mine;
    });
    for (const CellBox &b : part)
        box.merge(b);
    return box;
}

// `order` = the axes by falling extent of the world's box of cells (ties: x, y, z): see slab_key.  Returns the box.
CellBox slab_axes(const int64_t *keys, uint32_t n, int order[3])
{
    const CellBox box = box_of_keys(keys, n);
    order[0] = 0, order[1] = 1, order[2] = 2;
    if (n)
        std::stable_sort(order, order + 3, [&](int a, int b) { return box.hi[a] - box.lo[a] > box.hi[b] - box.lo[b]; });
    return box;
}

} // namespace

// The body sequence (slab key, id) is cut at positions t_r = the start of rank r's equal share.  K_r = the slab key at
// position t_r of the sorted sequence is found without sorting it: a histogram of the bodies per LAYER (the slab key's
// leading coordinate, the one the slabs are cut across) locates the layer position t_r falls in, and only that layer's
// bodies are gathered and sorted (a 1024-layer world: a thousandth of the bodies per cut).
void compute_owners(const int64_t *keys, uint32_t n, uint32_t w, uint8_t *owner, std::vector<Cut> &cuts, int axes[3])
{
    cuts.assign(w, Cut{INT64_MIN, 0});
    axes[0] = 0, axes[1] = 1, axes[2] = 2;
    if (n == 0)
        return;
    const CellBox box = slab_axes(keys, n, axes);
    std::vector<int64_t> slab(n);
    const int64_t layer_lo = box.lo[axes[0]];
    const size_t n_layers = (size_t)(box.hi[axes[0]] - layer_lo + 1);
    auto layer_of = [layer_lo](int64_t slab_key_) { return (size_t)(((slab_key_ >> 42) - kCellBias) - layer_lo); };
    const unsigned t_count = plan_threads(n);
    std::vector<std::vector<uint32_t>> hist(t_count, std::vector<uint32_t>(n_layers, 0));
    parallel_chunks(n, [&](unsigned t, size_t begin, size_t end) {
        uint32_t *h = hist[t].data();
        for (size_t g = begin; g < end; ++g) {
            slab[g] = slab_key(keys[g], axes);
            ++h[layer_of(slab[g])];
        }
    });
    if (w >= 2) {
        std::vector<uint64_t> first(n_layers + 1, 0); // bodies in the layers before layer x
        for (size_t x = 0; x < n_layers; ++x) {
            uint64_t c = 0;
            for (unsigned t = 0; t < t_count; ++t)
                c += hist[t][x];
            first[x + 1] = first[x] + c;
        }
        // the layer every cut position falls in; the bodies of those layers
        std::vector<size_t> cut_layer(w, SIZE_MAX);
        std::vector<int32_t> slot_of_layer(n_layers, -1);
        std::vector<std::vector<Cut>> members;
        for (uint32_t r = 1; r < w; ++r) {
            const size_t t = shard_range(n, r, w).first;
            if (t >= n)
                continue;
            const size_t x = (size_t)(std::upper_bound(first.begin(), first.end(), (uint64_t)t) - first.begin()) - 1;
            cut_layer[r] = x;
            if (slot_of_layer[x] < 0) {
                slot_of_layer[x] = (int32_t)members.size();
                members.emplace_back();
            }
        }
        std::vector<std::vector<std::vector<Cut>>> found(t_count, std::vector<std::vector<Cut>>(members.size()));
        parallel_chunks(n, [&](unsigned t, size_t begin, size_t end) {
            for (size_t g = begin; g < end; ++g) {
                const int32_t m = slot_of_layer[layer_of(slab[g])];
                if (m >= 0)
                    found[t][(size_t)m].push_back(Cut{slab[g], (uint32_t)g});
            }
        });
        for (size_t m = 0; m < members.size(); ++m) {
            for (unsigned t = 0; t < t_count; ++t)
                members[m].insert(members[m].end(), found[t][m].begin(), found[t][m].end());
            std::sort(members[m].begin(), members[m].end(), [](const Cut &a, const Cut &b) { return a.key < b.key || (a.key == b.key && a.id < b.id); });
        }
        const uint32_t share = std::max(1u, n / w);
        for (uint32_t r = 1; r < w; ++r) {
            const size_t t = shard_range(n, r, w).first; // bodies the ranks before r should own
            if (t >= n) {
                cuts[r] = Cut{INT64_MAX, UINT32_MAX};
                continue;
            }
            const std::vector<Cut> &layer = members[(size_t)slot_of_layer[cut_layer[r]]];
            const size_t base = (size_t)first[cut_layer[r]];
            const int64_t K = layer[t - base].key;
            const auto key_less = [](const Cut &c, int64_t k) { return c.key < k; };
            const size_t i_less = (size_t)(std::lower_bound(layer.begin(), layer.end(), K, key_less) - layer.begin());
            const size_t i_leq = (size_t)(std::lower_bound(layer.begin(), layer.end(), K + 1, key_less) - layer.begin());
            const size_t less = base + i_less, leq = base + i_leq;
            const size_t before = t - less, after = leq - t; // bodies of cell K on the wrong side if the cut goes before / after it
            if (std::min(before, after) * 4 <= share)
                cuts[r] = before <= after ? Cut{K, 0} : Cut{K + 1, 0};
            else // split cell K: its `before` lowest ids stay with the ranks before r
                cuts[r] = Cut{K, layer[i_less + before].id};
        }
        for (uint32_t r = 1; r < w; ++r) // monotone whatever the snapping did
            if (!(cuts[r - 1] <= cuts[r]))
                cuts[r] = cuts[r - 1];
    }
    parallel_chunks(n, [&](unsigned, size_t begin, size_t end) {
        for (size_t g = begin; g < end; ++g)
            owner[g] = (uint8_t)owner_of(cuts, slab[g], (uint32_t)g);
    });
}

// Everything hashed lies in the RIM of the rank's box: a per-axis occupancy of foreign cells picks the axis along which the
// fewest of the rank's layers have a foreign cell within two layers (the axis the slabs are cut across), and own bodies
// outside those layers -- nearly all of a slab -- are classified without a hash lookup.
void HaloPlanner::plan_lists(const std::vector<uint32_t> &own, const std::vector<int64_t> &own_keys, const std::vector<Foreign> &foreign,
                             const std::vector<CrossJoint> &cross, std::vector<uint32_t> &ghosts, std::vector<uint32_t> &boundary,
                             std::vector<uint8_t> *far)
{
    const uint32_t n_own = (uint32_t)own.size();
    const unsigned t_count = plan_threads(n_own);
    const CellBox box = box_of_keys(own_keys.data(), n_own);
    const int64_t *lo = box.lo, *hi = box.hi;
    // `layers[a]`: per coordinate of the box along axis a, is there a foreign cell?
    std::vector<uint8_t> layers[3];
    int64_t layer0[3] = {0, 0, 0};
    for (int a = 0; a < 3 && n_own; ++a) {
        layer0[a] = lo[a] - 4;
        layers[a].assign((size_t)(hi[a] - lo[a] + 9), 0);
    }
    std::unordered_set<int64_t> foreign_cells;
    std::vector<Foreign> candidates; // foreign bodies inside the box grown by one cell: the possible ghosts
    for (const Foreign &f : foreign) {
        if (!n_own)
            break;
        int64_t c[3];
        cell_of_key(f.key, c);
        bool in2 = true, in1 = true;
        for (int a = 0; a < 3; ++a) {
            in2 = in2 && c[a] >= lo[a] - 2 && c[a] <= hi[a] + 2;
            in1 = in1 && c[a] >= lo[a] - 1 && c[a] <= hi[a] + 1;
        }
        if (!in2)
            continue;
        foreign_cells.insert(f.key);
        for (int a = 0; a < 3; ++a)
            layers[a][(size_t)(c[a] - layer0[a])] = 1;
        if (in1)
            candidates.push_back(f);
    }
    // near1 / near2 [x]: a foreign cell within one / two layers of layer x, along the axis that leaves the smallest share
    // of the box near foreign layers
    int major = 0;
    std::vector<uint8_t> near1, near2;
    double best = 2.0;
    for (int a = 0; a < 3 && n_own; ++a) {
        std::vector<uint8_t> n1(layers[a].size(), 0), n2(layers[a].size(), 0);
        size_t marked = 0;
        for (size_t x = 0; x < layers[a].size(); ++x) {
            for (int d = -2; d <= 2; ++d) {
                const size_t y = x + (size_t)(d + 2);
                if (y < 2 || y - 2 >= layers[a].size() || !layers[a][y - 2])
                    continue;
                n2[x] = 1;
                if (d >= -1 && d <= 1)
                    n1[x] = 1;
            }
            marked += n2[x] && x >= 4 && x < layers[a].size() - 4;
        }
        const double share = (double)marked / (double)(hi[a] - lo[a] + 1);
        if (share < best) {
            best = share;
            major = a;
            near1.swap(n1);
            near2.swap(n2);
        }
    }
    const int64_t layer_base = layer0[major];
    // this rank's cells next to foreign layers (the rim): per cell, is a foreign body within one cell?  (then all its
    // bodies are boundary bodies)
    std::unordered_map<int64_t, uint8_t> rim_cells;
    std::vector<uint8_t> is_boundary(n_own, 0);
    // (which own bodies lie in layers near foreign ones: a pass over all of them, in a few threads; the hashing below is
    // for those only)
    std::vector<std::vector<uint32_t>> rim_part(t_count), near2_part(t_count);
    parallel_chunks(n_own, [&](unsigned t, size_t begin, size_t end) {
        for (size_t k = begin; k < end; ++k) {
            int64_t c[3];
            cell_of_key(own_keys[k], c);
            const size_t x = (size_t)(c[major] - layer_base);
            if (near1[x])
                rim_part[t].push_back((uint32_t)k);
            if (near2[x])
                near2_part[t].push_back((uint32_t)k);
        }
    });
    std::vector<uint32_t> rim_list, near2_list;
    for (unsigned t = 0; t < t_count; ++t) {
        rim_list.insert(rim_list.end(), rim_part[t].begin(), rim_part[t].end());
        near2_list.insert(near2_list.end(), near2_part[t].begin(), near2_part[t].end());
    }
    for (uint32_t k : rim_list) {
        int64_t c[3];
        cell_of_key(own_keys[k], c);
        auto it = rim_cells.find(own_keys[k]);
        if (it == rim_cells.end()) {
            bool seen = false;
            for (int dx = -1; dx <= 1 && !seen; ++dx)
                for (int dy = -1; dy <= 1 && !seen; ++dy)
                    for (int dz = -1; dz <= 1 && !seen; ++dz)
                        seen = foreign_cells.count(cell_key(c[0] + dx, c[1] + dy, c[2] + dz)) != 0;
            it = rim_cells.emplace(own_keys[k], seen).first;
        }
        is_boundary[k] = it->second;
    }
    // a candidate is a ghost iff an own cell lies within one cell of its cell (such an own cell is a rim cell)
    std::unordered_map<int64_t, uint8_t> reached; // foreign cell -> within one cell of an own cell (memoised)
    std::vector<uint32_t> ghost_list;
    for (const Foreign &f : candidates) {
        auto it = reached.find(f.key);
        if (it == reached.end()) {
            int64_t c[3];
            cell_of_key(f.key, c);
            bool near = false;
            for (int dx = -1; dx <= 1 && !near; ++dx)
                for (int dy = -1; dy <= 1 && !near; ++dy)
                    for (int dz = -1; dz <= 1 && !near; ++dz)
                        near = rim_cells.count(cell_key(c[0] + dx, c[1] + dy, c[2] + dz)) != 0;
            it = reached.emplace(f.key, near).first;
        }
        if (it->second)
            ghost_list.push_back(f.id);
    }
    for (const CrossJoint &j : cross) {
        ghost_list.push_back(j.remote_id);
        is_boundary[std::lower_bound(own.begin(), own.end(), j.own_id) - own.begin()] = 1;
    }
    std::sort(ghost_list.begin(), ghost_list.end());
    ghost_list.erase(std::unique(ghost_list.begin(), ghost_list.end()), ghost_list.end());
    ghosts.swap(ghost_list);
    boundary.clear();
    for (uint32_t k = 0; k < n_own; ++k)
        if (is_boundary[k])
            boundary.push_back(own[k]);
    if (far) {
        // an own body with a foreign cell within two cells of its own (or a boundary body) is not far
        far->assign(n_own, 0);
        const size_t limit = 20000; // beyond that many foreign cells around the slab the test is not worth it: nobody is far
        if (n_own && foreign_cells.size() <= limit) {
            std::unordered_map<int64_t, uint8_t> near_cells; // own cell in a layer near foreign ones -> a foreign cell within two cells
            for (uint32_t k = 0; k < n_own; ++k) // (outside those layers: far unless a joint made it a boundary body)
                (*far)[k] = !is_boundary[k];
            for (uint32_t k : near2_list) {
                int64_t c[3];
                cell_of_key(own_keys[k], c);
                auto it = near_cells.find(own_keys[k]);
                if (it == near_cells.end()) {
                    bool seen = false;
                    for (int dx = -2; dx <= 2 && !seen; ++dx)
                        for (int dy = -2; dy <= 2 && !seen; ++dy)
                            for (int dz = -2; dz <= 2 && !seen; ++dz)
                                seen = foreign_cells.count(cell_key(c[0] + dx, c[1] + dy, c[2] + dz)) != 0;
                    it = near_cells.emplace(own_keys[k], seen).first;
                }
                (*far)[k] = !it->second && !is_boundary[k];
            }
        }
    }
}

// Two passes over the world (in a few threads, see parallel_chunks) collect the rank's bodies and the foreign bodies within
// two cells of their box.
void HaloPlanner::plan_rank(const int64_t *keys, const uint8_t *owner, uint32_t n, uint32_t rank, const xpbd_joint *joints, uint32_t n_joints,
                            std::vector<uint32_t> &own, std::vector<uint32_t> &ghosts, std::vector<uint32_t> &boundary, std::vector<uint8_t> *far)
{
    own.clear();
    std::vector<int64_t> own_keys;
    CellBox box;
    const unsigned t_count = plan_threads(n);
    {
        std::vector<std::vector<uint32_t>> part(t_count);
        CellBox part_box[kPlanThreads];
        parallel_chunks(n, [&](unsigned t, size_t begin, size_t end) {
            CellBox b;
            std::vector<uint32_t> &mine = part[t];
            for (size_t g = begin; g < end; ++g)
                if (owner[g] == rank) {
                    mine.push_back((uint32_t)g);
                    b.add(keys[g]);
                }
            part_box[t] = b;
        });
        for (unsigned t = 0; t < t_count; ++t) {
            own.insert(own.end(), part[t].begin(), part[t].end());
            box.merge(part_box[t]);
        }
    }
    const int64_t *lo = box.lo, *hi = box.hi;
    own_keys.resize(own.size());
    for (size_t k = 0; k < own.size(); ++k)
        own_keys[k] = keys[own[k]];
    std::vector<Foreign> foreign;
    if (!own.empty()) {
        std::vector<std::vector<Foreign>> part(t_count);
        parallel_chunks(n, [&](unsigned t, size_t begin, size_t end) {
            for (size_t g = begin; g < end; ++g) {
                if (owner[g] == rank)
                    continue;
                int64_t c[3];
                cell_of_key(keys[g], c);
                bool in2 = true;
                for (int a = 0; a < 3; ++a)
                    in2 = in2 && c[a] >= lo[a] - 2 && c[a] <= hi[a] + 2;
                if (in2)
                    part[t].push_back(Foreign{(uint32_t)g, keys[g]});
            }
        });
        for (unsigned t = 0; t < t_count; ++t)
            foreign.insert(foreign.end(), part[t].begin(), part[t].end());
    }
    std::vector<CrossJoint> cross;
    for (uint32_t j = 0; j < n_joints; ++j) {
        const uint32_t a = joints[j].body_a, b = joints[j].body_b;
        const bool own_a = owner[a] == rank, own_b = owner[b] == rank;
        if (own_a && !own_b)
            cross.push_back(CrossJoint{a, b});
        else if (own_b && !own_a)
            cross.push_back(CrossJoint{b, a});
    }
    plan_lists(own, own_keys, foreign, cross, ghosts, boundary, far);
}

void exports_of(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<uint8_t> &held_owner, const std::vector<uint32_t> &boundary,
                std::vector<uint32_t> &exports)
{
    exports.clear();
    size_t b = 0;
    for (size_t i = 0; i < held_ids.size(); ++i) {
        const uint32_t g = held_ids[i];
        while (b < boundary.size() && boundary[b] < g)
            ++b;
        if (held_owner[i] != rank || (b < boundary.size() && boundary[b] == g))
            exports.push_back(g);
    }
}

std::vector<int64_t> cut_layers_of(const std::vector<Cut> &cuts)
{
    std::vector<int64_t> layers;
    for (size_t r = 1; r < cuts.size(); ++r)
        if (cuts[r].key != INT64_MAX)
            layers.push_back((cuts[r].key >> 42) - kCellBias);
    std::sort(layers.begin(), layers.end());
    layers.erase(std::unique(layers.begin(), layers.end()), layers.end());
    return layers;
}

void JointLists::build(const xpbd_joint *joints, uint32_t n_joints, uint32_t n_global)
{
    off.assign((size_t)n_global + 1, 0);
    for (uint32_t j = 0; j < n_joints; ++j)
        ++off[joints[j].body_a + 1], ++off[joints[j].body_b + 1];
    for (uint32_t g = 0; g < n_global; ++g)
        off[g + 1] += off[g];
    adj.assign((size_t)2 * n_joints, 0);
    std::vector<uint32_t> cursor(off.begin(), off.end() - 1);
    for (uint32_t j = 0; j < n_joints; ++j) {
        adj[cursor[joints[j].body_a]++] = j;
        adj[cursor[joints[j].body_b]++] = j;
    }
}

void rim_rows_of(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<int64_t> &held_keys, const std::vector<uint8_t> &held_owner,
                 const std::vector<int64_t> &held_slab, const std::vector<int64_t> &cut_layers, const JointIndex &ji, std::vector<int32_t> &slot_of,
                 std::vector<RimRow> &rows)
{
    auto near_a_cut = [&](int64_t slab) {
        const int64_t layer = (slab >> 42) - kCellBias;
        const auto at = std::lower_bound(cut_layers.begin(), cut_layers.end(), layer - 2);
        return at != cut_layers.end() && *at <= layer + 2;
    };
    if (ji.any) // (scratch: where in the held lists a body of this shard sits)
        for (size_t i = 0; i < held_ids.size(); ++i)
            slot_of[held_ids[i]] = (int32_t)i;
    for (size_t i = 0; i < held_ids.size(); ++i) {
        const uint32_t g = held_ids[i];
        bool publish = held_owner[i] != rank || near_a_cut(held_slab[i]);
        for (uint32_t e = ji.any ? ji.off[g] : 0u; ji.any && e < ji.off[g + 1] && !publish; ++e) {
            const xpbd_joint &j = ji.joints[ji.adj[e]];
            const int32_t at = slot_of[j.body_a == g ? j.body_b : j.body_a];
            // the other end lives elsewhere now, or will: this end's owner (or mirror) must learn about both
            publish = at < 0 || held_owner[(size_t)at] != held_owner[i];
        }
        if (publish)
            rows.push_back(RimRow{held_keys[i], g, held_owner[i], {0, 0, 0}});
    }
    if (ji.any)
        for (size_t i = 0; i < held_ids.size(); ++i)
            slot_of[held_ids[i]] = -1;
}

int light_rank_plan(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<int64_t> &held_keys, const std::vector<uint8_t> &held_owner,
                    KnownMap &known, const JointIndex &ji, std::vector<int32_t> &slot_of, ShardPlan &pl)
{
    std::vector<std::pair<uint32_t, int64_t>> arriving;
    std::vector<HaloPlanner::Foreign> foreign;
    for (const auto &kv : known) {
        if (kv.second.owner == rank) {
            if (kv.second.holder != rank)
                arriving.emplace_back(kv.first, kv.second.key);
        } else {
            foreign.push_back(HaloPlanner::Foreign{kv.first, kv.second.key});
        }
    }
    std::sort(arriving.begin(), arriving.end());
    std::vector<int64_t> own_keys;
    pl.own.reserve(held_ids.size() + arriving.size());
    own_keys.reserve(held_ids.size() + arriving.size());
    size_t ai = 0;
    for (size_t i = 0; i <= held_ids.size(); ++i) {
        const uint32_t g = i < held_ids.size() ? held_ids[i] : UINT32_MAX;
        for (; ai < arriving.size() && arriving[ai].first < g; ++ai) {
            pl.own.push_back(arriving[ai].first);
            own_keys.push_back(arriving[ai].second);
            pl.own_holder.push_back(known[arriving[ai].first].holder);
        }
        if (i < held_ids.size() && held_owner[i] == rank) {
            pl.own.push_back(g);
            own_keys.push_back(held_keys[i]);
            pl.own_holder.push_back((uint8_t)rank);
        }
    }
    // joints that leave the rank: the other end was published by its holder (or is held here and goes elsewhere)
    std::vector<HaloPlanner::CrossJoint> cross;
    int rc = XPBD_OK;
    if (ji.any) {
        for (uint32_t g : pl.own)
            slot_of[g] = 0; // (scratch: the bodies the shard will own)
        for (uint32_t g : pl.own) {
            for (uint32_t e = ji.off[g]; e < ji.off[g + 1] && rc == XPBD_OK; ++e) {
                const xpbd_joint &j = ji.joints[ji.adj[e]];
                const uint32_t other = j.body_a == g ? j.body_b : j.body_a;
                if (slot_of[other] >= 0)
                    continue;
                if (!known.count(other)) {
                    rc = set_error(XPBD_E_HIP, "xpbd_multi_world: body %u (joint %u) is in nobody's rim (inconsistent plans)", other, ji.adj[e]);
                    break;
                }
                cross.push_back(HaloPlanner::CrossJoint{g, other});
            }
        }
        for (uint32_t g : pl.own)
            slot_of[g] = -1;
    }
    if (rc != XPBD_OK)
        return rc;
    HaloPlanner::plan_lists(pl.own, own_keys, foreign, cross, pl.ghosts, pl.boundary, &pl.far);
    pl.ghost_owner.resize(pl.ghosts.size());
    pl.ghost_holder.resize(pl.ghosts.size());
    for (size_t i = 0; i < pl.ghosts.size(); ++i) {
        const Known &kn = known[pl.ghosts[i]];
        pl.ghost_owner[i] = kn.owner, pl.ghost_holder[i] = kn.holder;
    }
    return XPBD_OK;
}

void full_rank_plan(uint32_t rank, const std::vector<uint32_t> &held_ids, const int64_t *keys, const uint8_t *owner, const uint8_t *holder, uint32_t n,
                    const xpbd_joint *joints, uint32_t n_joints, ShardPlan &pl)
{
    HaloPlanner::plan_rank(keys, owner, n, rank, joints, n_joints, pl.own, pl.ghosts, pl.boundary, &pl.far);
    pl.own_holder.resize(pl.own.size());
    for (size_t i = 0; i < pl.own.size(); ++i)
        pl.own_holder[i] = holder[pl.own[i]];
    pl.ghost_owner.resize(pl.ghosts.size());
    pl.ghost_holder.resize(pl.ghosts.size());
    for (size_t i = 0; i < pl.ghosts.size(); ++i)
        pl.ghost_owner[i] = owner[pl.ghosts[i]], pl.ghost_holder[i] = holder[pl.ghosts[i]];
    std::vector<uint8_t> held_owner(held_ids.size());
    for (size_t i = 0; i < held_ids.size(); ++i)
        held_owner[i] = owner[held_ids[i]];
    exports_of(rank, held_ids, held_owner, pl.boundary, pl.exports);
}

int layout_shard(uint32_t rank, const ShardPlan &pl, const std::vector<uint32_t> &held_ids, const std::vector<uint32_t> &held_slots, const RankIds &boundary,
                 const RankIds &exports, uint32_t rows, const JointIndex &ji, std::vector<int32_t> &slot_of, double margin, double edge, ShardLayout &out)
{
    const uint32_t n_own = (uint32_t)pl.own.size(), n_ghost = (uint32_t)pl.ghosts.size(), n_loc = n_own + n_ghost;
    out = ShardLayout();
    out.local_ids.resize(n_loc);
    out.src.resize(n_loc);
    out.owned_slots.resize(n_own);
    out.ghost_slots.resize(n_ghost);
    out.ghost_rows.resize(n_ghost);
    // owned + ghost bodies in ascending global id.  A body the shard owned before and still owns moves on the device; a body
    // that arrives (a new owner, a ghost) comes from its holder's exported record.
    uint32_t slot = 0, oi = 0, gi = 0;
    size_t old = 0; // walks the bodies held so far (ascending, like pl.own)
    while (oi < n_own || gi < n_ghost) {
        const bool take_own = gi >= n_ghost || (oi < n_own && pl.own[oi] < pl.ghosts[gi]);
        const uint32_t g = take_own ? pl.own[oi] : pl.ghosts[gi];
        out.local_ids[slot] = g;
        if (take_own && pl.own_holder[oi] == rank) {
            while (old < held_ids.size() && held_ids[old] < g)
                ++old;
            if (old == held_ids.size() || held_ids[old] != g)
                return set_error(XPBD_E_HIP, "xpbd_multi_world: body %u is not among the bodies rank %u holds (inconsistent plans)", g, rank);
            out.src[slot] = (int32_t)held_slots[old];
        } else {
            const uint32_t h = take_own ? pl.own_holder[oi] : pl.ghost_holder[gi];
            const int64_t at = exports.find(h, g);
            if (at < 0)
                return set_error(XPBD_E_HIP, "xpbd_multi_world: body %u is needed by rank %u but not exported by its holder %u (inconsistent plans)", g, rank, h);
            out.incoming.push_back(ShardLayout::Incoming{h, (uint32_t)at});
            out.src[slot] = -(int32_t)out.incoming.size();
        }
        if (take_own) {
            out.owned_slots[oi++] = slot;
        } else {
            const uint32_t o = pl.ghost_owner[gi];
            const int64_t at = boundary.find(o, g);
            if (at < 0)
                return set_error(XPBD_E_HIP, "xpbd_multi_world: body %u is mirrored by rank %u but not exported by its owner %u (inconsistent plans)", g, rank, o);
            out.ghost_slots[gi] = slot;
            out.ghost_rows[gi] = o * rows + (uint32_t)at;
            ++gi;
        }
        ++slot;
    }
    out.boundary_slots.resize(pl.boundary.size());
    for (size_t q = 0; q < pl.boundary.size(); ++q)
        out.boundary_slots[q] = out.owned_slots[std::lower_bound(pl.own.begin(), pl.own.end(), pl.boundary[q]) - pl.own.begin()];
    out.skip.assign(n_loc, 0);
    out.owned.assign(n_loc, 1);
    out.query_ids = out.local_ids;
    for (uint32_t q : out.boundary_slots)
        out.skip[q] = 1;
    for (uint32_t q : out.ghost_slots)
        out.skip[q] = 1, out.owned[q] = 0, out.query_ids[q] = XPBD_NO_HIT;
    // joints whose two bodies are both present here, in global joint order, re-indexed to local slots: the joints of the
    // local bodies through the per-body joint lists (a joint is taken at its lower-numbered end)
    for (uint32_t q = 0; q < n_loc; ++q)
        slot_of[out.local_ids[q]] = (int32_t)q;
    for (uint32_t q = 0; q < n_loc && ji.any; ++q) {
        const uint32_t g = out.local_ids[q];
        for (uint32_t e = ji.off[g]; e < ji.off[g + 1]; ++e) {
            const xpbd_joint &j = ji.joints[ji.adj[e]];
            const uint32_t other = j.body_a == g ? j.body_b : j.body_a;
            if (slot_of[other] >= 0 && (g < other || (g == other && j.body_a == g)))
                out.joint_ids.push_back(ji.adj[e]);
        }
    }
    std::sort(out.joint_ids.begin(), out.joint_ids.end());
    out.joint_ids.erase(std::unique(out.joint_ids.begin(), out.joint_ids.end()), out.joint_ids.end());
    out.joints.resize(out.joint_ids.size());
    for (size_t q = 0; q < out.joint_ids.size(); ++q) {
        xpbd_joint l = ji.joints[out.joint_ids[q]];
        l.body_a = (uint32_t)slot_of[l.body_a];
        l.body_b = (uint32_t)slot_of[l.body_b];
        out.joints[q] = l;
    }
    for (uint32_t q = 0; q < n_loc; ++q)
        slot_of[out.local_ids[q]] = -1;
    // 1 / allowance^2 per owned body: the displacement check then yields the largest FRACTION of its allowance any body has used
    const double near_allow = margin, far_allow = margin + 0.5 * edge;
    const double near_scale = 1.0 / (near_allow * near_allow), far_scale = 1.0 / (far_allow * far_allow);
    out.disp_scale.resize(n_own);
    for (uint32_t i = 0; i < n_own; ++i)
        out.disp_scale[i] = pl.far[i] ? far_scale : near_scale;
    return XPBD_OK;
}

namespace {
// Ownership by contiguous index ranges (what a caller that orders its bodies itself would get).
void range_owners(uint32_t n_global, uint32_t n_ranks, std::vector<uint8_t> &owner)
{
    owner.resize(n_global);
    for (uint32_t r = 0; r < n_ranks; ++r) {
        const Range rr = shard_range(n_global, r, n_ranks);
        std::fill(owner.begin() + rr.first, owner.begin() + rr.first + rr.count, (uint8_t)r);
    }
}
} // namespace

} // namespace plan
} // namespace xpbd

using namespace xpbd::plan;
using xpbd::set_error;

extern "C" {

// Diagnostics (host only, no device): ownership and halo plans from the global cell keys, as the plans of xpbd_multi.cpp compute them.
int xpbd_halo_partition(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint8_t *owner)
try {
    if ((n_global && (!cell_keys || !owner)) || n_ranks == 0 || n_ranks > 64)
        return set_error(XPBD_E_INVALID, "xpbd_halo_partition: bad argument");
    std::vector<Cut> cuts;
    int axes[3];
    compute_owners(cell_keys, n_global, n_ranks, owner, cuts, axes);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_halo_plan_light(const int64_t *keys_at_cut, const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank,
                         const xpbd_joint *joints, uint32_t n_joints, uint8_t *owner_now, uint32_t *own, uint32_t *n_own, uint32_t *ghosts,
                         uint32_t *n_ghosts, uint32_t *boundary, uint32_t *n_boundary, uint8_t *far, uint32_t cap)
try {
    if (!keys_at_cut || !cell_keys || !owner_now || !n_own || !n_ghosts || !n_boundary || n_ranks == 0 || n_ranks > 64 || rank >= n_ranks ||
        (n_joints && !joints) || (cap && (!own || !ghosts || !boundary)))
        return set_error(XPBD_E_INVALID, "xpbd_halo_plan_light: bad argument");
    for (uint32_t j = 0; j < n_joints; ++j)
        if (joints[j].body_a >= n_global || joints[j].body_b >= n_global)
            return set_error(XPBD_E_INVALID, "xpbd_halo_plan_light: joint %u names a body out of range", j);
    // the cuts of the last full plan; who holds what since
    std::vector<Cut> cuts;
    int axes[3];
    std::vector<uint8_t> holder(n_global);
    compute_owners(keys_at_cut, n_global, n_ranks, holder.data(), cuts, axes);
    JointLists joint_lists; // the joints at every body
    joint_lists.build(joints, n_joints, n_global);
    const JointIndex ji = joint_lists.view(joints);
    // every rank: the bodies it holds, their owners from the kept cuts, its rim
    const std::vector<int64_t> cut_layers = cut_layers_of(cuts);
    std::vector<int32_t> slot_of(n_global, -1);
    std::vector<std::vector<uint32_t>> held_ids(n_ranks);
    std::vector<std::vector<int64_t>> held_keys(n_ranks), held_slab(n_ranks);
    std::vector<std::vector<uint8_t>> held_owner(n_ranks);
    for (uint32_t g = 0; g < n_global; ++g) {
        const uint32_t h = holder[g];
        const int64_t slab = slab_key(cell_keys[g], axes);
        owner_now[g] = (uint8_t)owner_of(cuts, slab, g);
        held_ids[h].push_back(g);
        held_keys[h].push_back(cell_keys[g]);
        held_slab[h].push_back(slab);
        held_owner[h].push_back(owner_now[g]);
    }
    KnownMap known;
    for (uint32_t h = 0; h < n_ranks; ++h) {
        std::vector<RimRow> rows;
        rim_rows_of(h, held_ids[h], held_keys[h], held_owner[h], held_slab[h], cut_layers, ji, slot_of, rows);
        for (const RimRow &r : rows)
            known.emplace(r.id, Known{r.key, r.owner, (uint8_t)h});
    }
    ShardPlan pl;
    if (int rc = light_rank_plan(rank, held_ids[rank], held_keys[rank], held_owner[rank], known, ji, slot_of, pl))
        return rc;
    *n_own = (uint32_t)pl.own.size(), *n_ghosts = (uint32_t)pl.ghosts.size(), *n_boundary = (uint32_t)pl.boundary.size();
    if (pl.own.size() > cap || pl.ghosts.size() > cap || pl.boundary.size() > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_halo_plan_light: %zu owned, %zu ghosts, %zu boundary bodies, capacity %u", pl.own.size(), pl.ghosts.size(),
                         pl.boundary.size(), cap);
    std::copy(pl.own.begin(), pl.own.end(), own);
    std::copy(pl.ghosts.begin(), pl.ghosts.end(), ghosts);
    std::copy(pl.boundary.begin(), pl.boundary.end(), boundary);
    if (far)
        std::copy(pl.far.begin(), pl.far.end(), far);
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_halo_plan_owned(const int64_t *cell_keys, const uint8_t *owner, uint32_t n_global, uint32_t n_ranks, uint32_t rank, const xpbd_joint *joints,
                         uint32_t n_joints, uint32_t *ghosts, uint32_t *n_ghosts, uint32_t *boundary, uint32_t *n_boundary, uint8_t *far, uint32_t cap)
try {
    if (!cell_keys || !owner || !n_ghosts || !n_boundary || n_ranks == 0 || n_ranks > 64 || rank >= n_ranks || (n_joints && !joints) ||
        (cap && (!ghosts || !boundary)))
        return set_error(XPBD_E_INVALID, "xpbd_halo_plan_owned: bad argument");
    for (uint32_t g = 0; g < n_global; ++g)
        if (owner[g] >= n_ranks)
            return set_error(XPBD_E_INVALID, "xpbd_halo_plan_owned: owner[%u] = %u of %u ranks", g, owner[g], n_ranks);
    for (uint32_t j = 0; j < n_joints; ++j)
        if (joints[j].body_a >= n_global || joints[j].body_b >= n_global)
            return set_error(XPBD_E_INVALID, "xpbd_halo_plan_owned: joint %u names a body out of range", j);
    std::vector<uint32_t> own, g, b;
    std::vector<uint8_t> f;
    HaloPlanner::plan_rank(cell_keys, owner, n_global, rank, joints, n_joints, own, g, b, far ? &f : nullptr);
    *n_ghosts = (uint32_t)g.size(), *n_boundary = (uint32_t)b.size();
    if (g.size() > cap || b.size() > cap || (far && f.size() > cap))
        return set_error(XPBD_E_CAPACITY, "xpbd_halo_plan_owned: %zu ghosts, %zu boundary bodies, %zu owned, capacity %u", g.size(), b.size(), own.size(), cap);
    std::copy(g.begin(), g.end(), ghosts);
    std::copy(b.begin(), b.end(), boundary);
    if (far)
        std::copy(f.begin(), f.end(), far); // one flag per owned body, in ascending id
    return XPBD_OK;
} XPBD_ABI_CATCH

// ... with ownership by contiguous index ranges
int xpbd_halo_plan(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank, const xpbd_joint *joints, uint32_t n_joints,
                   uint32_t *ghosts, uint32_t *n_ghosts, uint32_t *boundary, uint32_t *n_boundary, uint32_t cap)
try {
    if (n_ranks == 0 || n_ranks > 64)
        return set_error(XPBD_E_INVALID, "xpbd_halo_plan: bad argument");
    std::vector<uint8_t> owner;
    range_owners(n_global, n_ranks, owner);
    return xpbd_halo_plan_owned(cell_keys, owner.data(), n_global, n_ranks, rank, joints, n_joints, ghosts, n_ghosts, boundary, n_boundary, nullptr, cap);
} XPBD_ABI_CATCH

int xpbd_halo_plan_far(const int64_t *cell_keys, uint32_t n_global, uint32_t n_ranks, uint32_t rank, uint8_t *far, uint32_t cap, uint32_t *n_owned)
try {
    if (!cell_keys || !n_owned || n_ranks == 0 || n_ranks > 64 || rank >= n_ranks || (cap && !far))
        return set_error(XPBD_E_INVALID, "xpbd_halo_plan_far: bad argument");
    std::vector<uint8_t> owner;
    range_owners(n_global, n_ranks, owner);
    std::vector<uint32_t> own, g, b;
    std::vector<uint8_t> f;
    HaloPlanner::plan_rank(cell_keys, owner.data(), n_global, rank, nullptr, 0, own, g, b, &f);
    *n_owned = (uint32_t)f.size();
    if (f.size() > cap)
        return set_error(XPBD_E_CAPACITY, "xpbd_halo_plan_far: %zu owned bodies, capacity %u", f.size(), cap);
    std::copy(f.begin(), f.end(), far);
    return XPBD_OK;
} XPBD_ABI_CATCH

int64_t xpbd_halo_cell_key(const double centre[3], double cell_edge) noexcept
{
    if (!centre || !(cell_edge > 0.0))
        return 0;
    return cell_key(clamp_cell(std::floor(centre[0] / cell_edge)), clamp_cell(std::floor(centre[1] / cell_edge)), clamp_cell(std::floor(centre[2] / cell_edge)));
}

} // extern "C"
