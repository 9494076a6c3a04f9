// xpbd_plan.hpp -- the shard planner of the multi-GPU world (xpbd_multi.cpp): who owns which body, who mirrors whom.
//
// A pure function of cell keys, owners and joints: host only, no device, nothing but the standard library, include/xpbd.h and
// xpbd_error.h (tests/plan_standalone_main.cpp builds it with g++ alone).  Also behind the diagnostics xpbd_halo_* of the C ABI.
//
// Ownership is the LIBRARY's: the bodies are binned into the cells of a uniform grid (edge = 2 * (largest bounding radius +
// pad + halo_margin)), the cells are ordered by their spatial-hash cell key taken along the LONGEST axis of the world first,
// and that sequence is cut into n_ranks runs of near-equal body count -- every rank owns a slab of space across the world's
// longest axis, whatever order the caller numbered its bodies in.  A FULL plan cuts the slabs from the keys of the whole world
// (compute_owners, HaloPlanner::plan_rank); a LIGHT plan keeps the cuts, gives every body the owner its own key names
// (owner_of) and needs only the RIMS of the shards (rim_rows_of, light_rank_plan).
#pragma once

#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/xpbd.h"

namespace xpbd {
namespace plan __attribute__((visibility("hidden"))) { // (C++ names of the planner are not part of the library's ABI)

constexpr int64_t kCellBias = 1 << 20;
constexpr int64_t kCellLimit = kCellBias - 4; // |cell| <= this: the +-2 dilations of the planner stay inside the 21-bit fields

struct Range {
    uint32_t first, count;
};

// The index slice of the caller's bodies a rank HANDS OVER at upload: contiguous ranges, the first n % w ranks one body
// longer (constraint_solver_amd/sharding.py).  It says nothing about ownership.
inline Range shard_range(uint32_t n, uint32_t rank, uint32_t w)
{
    const uint32_t base = n / w, extra = n % w;
    return Range{rank * base + std::min(rank, extra), base + (rank < extra ? 1u : 0u)};
}

// x-major: ascending keys are slabs along x, inside a slab rows along y, inside a row columns along z
inline int64_t cell_key(int64_t x, int64_t y, int64_t z) { return ((x + kCellBias) << 42) | ((y + kCellBias) << 21) | (z + kCellBias); }

inline void cell_of_key(int64_t key, int64_t c[3])
{
    c[0] = (key >> 42) - kCellBias;
    c[1] = ((key >> 21) & ((1 << 21) - 1)) - kCellBias;
    c[2] = (key & ((1 << 21) - 1)) - kCellBias;
}

// ---- ownership: the x-major sequence of grid cells cut into n_ranks runs of near-equal body count ----------------------------
// A cut is a (cell key, body id) pair; rank r owns the bodies whose (key, id) lies in [cut[r], cut[r + 1]).  Cuts fall on
// cell boundaries (whole cells stay together) unless that would leave a rank more than a quarter of its share off balance
// (many bodies in one cell: a tiny world), in which case the cell is split by body id.
struct Cut {
    int64_t key;
    uint32_t id;
    bool operator<=(const Cut &o) const { return key < o.key || (key == o.key && id <= o.id); }
};

// The slabs are cut ACROSS THE LONGEST AXIS of the world's box of cells (a world 64 cells by 256 gets four slabs of 64 x 64,
// not of 16 x 256: a quarter of the boundary): `order` = the axes by falling extent (ties: x, y, z), and the bodies are
// sequenced by their cell key re-packed with the axes in that order.
inline int64_t slab_key(int64_t key, const int order[3])
{
    int64_t c[3];
    cell_of_key(key, c);
    return cell_key(c[order[0]], c[order[1]], c[order[2]]);
}

// Ownership of all bodies from their cell keys: owner[g], and the cuts (cuts[r] for r = 1 .. w - 1 over the SLAB keys,
// cuts[0] = the smallest possible pair); a deterministic function of the keys alone.
void compute_owners(const int64_t *keys, uint32_t n, uint32_t w, uint8_t *owner, std::vector<Cut> &cuts, int axes[3]);

inline uint32_t owner_of(const std::vector<Cut> &cuts, int64_t slab, uint32_t id)
{
    // number of cuts <= (key, id), minus one; cuts[0] is the smallest pair
    uint32_t lo = 0, hi = (uint32_t)cuts.size(); // cuts[lo] <= pair < cuts[hi]
    const Cut me{slab, id};
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (cuts[mid] <= me)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Which remote bodies a rank mirrors and which of its own bodies the others mirror; a pure function of the cell keys, the
// owners and the joints, so every rank computes consistent plans.
//   ghosts:   remote bodies in a cell within one cell of a cell this rank owns a body in (ascending);
//   boundary: this rank's bodies in a cell within one cell of a cell another rank owns a body in (ascending).
//   A joint between an owned and a remote body puts the remote one among the ghosts and the owned one on the boundary.
//   far (optional, one flag per owned body): no cell within two cells of the body's holds a foreign body.  Such a body
//   may travel halo_margin + edge / 2 before it can meet a body this rank does not mirror (any foreign body starts more
//   than two cell edges away, and 2 * (margin + edge / 2) = edge + 2 * margin is less than the 2 * edge - 2 r - pad the
//   two would have to close), the others halo_margin.
struct HaloPlanner {
    struct Foreign {
        uint32_t id;
        int64_t key;
    };
    struct CrossJoint { // a joint between one of the rank's bodies and a remote one
        uint32_t own_id, remote_id;
    };

    // The plan from LISTS: the rank's bodies (ascending ids) with their cell keys, the foreign bodies that may matter (any
    // superset of those within two cells of the box of the rank's cells), the joints that leave the rank.
    static void plan_lists(const std::vector<uint32_t> &own, const std::vector<int64_t> &own_keys, const std::vector<Foreign> &foreign,
                           const std::vector<CrossJoint> &cross, std::vector<uint32_t> &ghosts, std::vector<uint32_t> &boundary,
                           std::vector<uint8_t> *far);
    // ... and from the cell keys and owners of ALL n bodies of the world (a full plan, the host-only diagnostics): `own` = the
    // bodies of `rank` (ascending).
    static void plan_rank(const int64_t *keys, const uint8_t *owner, uint32_t n, uint32_t rank, const xpbd_joint *joints, uint32_t n_joints,
                          std::vector<uint32_t> &own, std::vector<uint32_t> &ghosts, std::vector<uint32_t> &boundary, std::vector<uint8_t> *far = nullptr);
};

// The new plan of one shard: what it will own (ascending ids) and who holds those bodies now, its ghosts / boundary / far
// lists, who owns and who holds its ghosts, what it hands out (bodies that change owner, bodies others mirror).
struct ShardPlan {
    std::vector<uint32_t> own, exports;
    std::vector<uint8_t> own_holder, ghost_owner, ghost_holder;
    std::vector<uint32_t> ghosts, boundary;
    std::vector<uint8_t> far;
};

// What a rank holds and somebody else needs: bodies that change owner, and its (remaining) bodies that others mirror.
// held_owner[i] = new owner of held body held_ids[i]; boundary = the rank's NEW boundary list (ascending).
void exports_of(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<uint8_t> &held_owner, const std::vector<uint32_t> &boundary,
                std::vector<uint32_t> &exports);

// ---- the pieces of a light plan ------------------------------------------------------------------------------------------------
struct RimRow { // what a holder publishes of a body: its cell key, its id, its new owner
    int64_t key;
    uint32_t id;
    uint8_t owner, pad[3];
};
struct Known { // ... and what everybody then knows of it
    int64_t key;
    uint8_t owner, holder;
};
using KnownMap = std::unordered_map<uint32_t, Known>;
struct JointIndex { // the joints of the world and, per body, the joints it is an end of (ascending joint index)
    const xpbd_joint *joints;
    const uint32_t *off, *adj;
    bool any;
};
struct JointLists { // ... owned: off [n_global + 1], adj [2 * n_joints] (indices into `joints`)
    std::vector<uint32_t> off, adj;
    void build(const xpbd_joint *joints, uint32_t n_joints, uint32_t n_global);
    JointIndex view(const xpbd_joint *joints) const { return JointIndex{joints, off.data(), adj.data(), !adj.empty()}; }
};

std::vector<int64_t> cut_layers_of(const std::vector<Cut> &cuts);

// The RIM a holder publishes: its bodies within two layers of a cut (no body further from every cut can lie within two cells
// of a foreign cell: a rank's bodies and a foreign body near them sit on opposite sides of a cut layer), the bodies that
// change owner, and the ends of joints that leave the shard (the other end is held elsewhere, or the two ends get different
// owners).  slot_of: [n_global] scratch, -1 everywhere on entry and on return.
void rim_rows_of(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<int64_t> &held_keys, const std::vector<uint8_t> &held_owner,
                 const std::vector<int64_t> &held_slab, const std::vector<int64_t> &cut_layers, const JointIndex &ji, std::vector<int32_t> &slot_of,
                 std::vector<RimRow> &rows);

// One rank's new plan from the bodies it holds and everybody's rims: what it will own (the held bodies that stay and the
// published bodies that come to it), its ghosts / boundary / far lists, who owns and holds the ghosts.
int light_rank_plan(uint32_t rank, const std::vector<uint32_t> &held_ids, const std::vector<int64_t> &held_keys, const std::vector<uint8_t> &held_owner,
                    KnownMap &known, const JointIndex &ji, std::vector<int32_t> &slot_of, ShardPlan &pl);

// ... and the same plan from the keys, owners and holders of ALL n bodies of the world (a full plan).
void full_rank_plan(uint32_t rank, const std::vector<uint32_t> &held_ids, const int64_t *keys, const uint8_t *owner, const uint8_t *holder, uint32_t n,
                    const xpbd_joint *joints, uint32_t n_joints, ShardPlan &pl);

// ---- the layout of a shard: a plan turned into local slots -----------------------------------------------------------------------
// The id lists of all ranks as gathered: rank r's counts[r] ids (ascending) start at ids[r * width].
struct RankIds {
    const uint32_t *ids, *counts;
    uint32_t width, n_ranks;
    int64_t find(uint32_t rank, uint32_t g) const // where g stands in the list of `rank`, or -1 (no such rank, not listed)
    {
        if (rank >= n_ranks || counts[rank] == 0)
            return -1;
        const uint32_t *lo = ids + (size_t)rank * width, *hi = lo + counts[rank], *at = std::lower_bound(lo, hi, g);
        return at != hi && *at == g ? (int64_t)(at - lo) : -1;
    }
};

// A shard's local world under a plan: its owned bodies and its ghosts in ascending global id, one slot each.
struct ShardLayout {
    struct Incoming { // where the record of a body that arrives lies: its holder, its place in the holder's export list
        uint32_t holder, row;
    };
    std::vector<uint32_t> local_ids;                  // global id of every slot
    std::vector<uint32_t> owned_slots, ghost_slots;   // slot of pl.own[i], of pl.ghosts[i]
    std::vector<uint32_t> ghost_rows;                 // row of pl.ghosts[i] in the per-substep all-gather: owner * rows + place on its boundary list
    std::vector<uint32_t> boundary_slots;             // slot of pl.boundary[i]
    std::vector<uint8_t> skip;                        // per slot: 1 for boundary bodies and ghosts (what the interior launch leaves out)
    std::vector<uint8_t> owned;                       // per slot: 1 for owned bodies, 0 for ghosts
    std::vector<uint32_t> query_ids;                  // per slot: local_ids, XPBD_NO_HIT for the ghosts (the owned bodies answer scene queries)
    std::vector<int32_t> src;                         // per slot: the slot the body has now (it stays on this shard), or -(k + 1) for the k-th arrival
    std::vector<Incoming> incoming;                   // the arrivals, in slot order
    std::vector<uint32_t> joint_ids;                  // global joints (ascending) with both ends here
    std::vector<xpbd_joint> joints;                   // ... re-indexed to slots: local joint q = joint_ids[q]
    std::vector<double> disp_scale;                   // per owned body: 1 / allowance^2 (allowance: margin, or margin + edge / 2 where pl.far)
};

// held_ids / held_slots: the bodies the shard holds now (ascending) and their slots; boundary / exports: those lists of every
// rank's NEW plan; rows: rows per rank of the per-substep all-gather.  slot_of: [n_global] scratch, -1 everywhere on entry and
// on return.  XPBD_E_HIP ("inconsistent plans") if the plans of the ranks do not fit together; `out` is unspecified then.
int layout_shard(uint32_t rank, const ShardPlan &pl, const std::vector<uint32_t> &held_ids, const std::vector<uint32_t> &held_slots, const RankIds &boundary,
                 const RankIds &exports, uint32_t rows, const JointIndex &ji, std::vector<int32_t> &slot_of, double margin, double edge, ShardLayout &out);

// The slot of global body g among local_ids (ascending), or -1.
inline int32_t slot_in_shard(const std::vector<uint32_t> &local_ids, uint32_t g)
{
    const auto at = std::lower_bound(local_ids.begin(), local_ids.end(), g);
    return at != local_ids.end() && *at == g ? (int32_t)(at - local_ids.begin()) : -1;
}

// The records (joint limits or drives: both name a joint in .joint) on the joints of a shard (joint_ids, ascending), re-indexed
// to the shard's joint numbering; the caller's order is kept.
template <class Record> std::vector<Record> local_joint_records(const std::vector<Record> &global, const std::vector<uint32_t> &joint_ids)
{
    std::vector<Record> local;
    for (const Record &r : global) {
        const int32_t q = slot_in_shard(joint_ids, r.joint);
        if (q >= 0) {
            local.push_back(r);
            local.back().joint = (uint32_t)q;
        }
    }
    return local;
}

} // namespace plan
} // namespace xpbd
