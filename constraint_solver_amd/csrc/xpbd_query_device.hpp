// xpbd_query_device.hpp -- scene queries (EXTENSION): the device-side routines that more than one family of queries uses.  Not
// installed, and included only by the query units (xpbd_query_grid.hip, _rays.hip, _overlap.hip, _sweep.hip, _distance.hip)
// through xpbd_query_units.hpp.  Everything is in an anonymous namespace, as it was when the families shared one unit: every
// unit gets its own copy, the kernels that use a routine see it exactly as before, and no symbol crosses a unit.
//
// Who uses what (a routine a family reaches only through another one of this header counts):
//
//   routine                                          grid  rays  overlap  sweep  distance
//   kBlock, QueryGrid, kEmpty / kGrid / kEveryBody     x     x      x       x       x
//   kBruteRays, kBruteBlocks                           x     x                          (grid: the scratch sizing)
//   kEdgeScale, kPadScale, kMaxCell, kMaxDim           x                                (what the walks below rely on)
//   Best, better, no_hit                               x     x              x       x   (grid: sizeof(Best))
//   load_body                                          x     x
//   query_key, clamp_axis                              x     x      x       x       x
//   clip_to_grid, next_face                                  x              x
//   kOverlapRecDoubles                                 x            x       x       x   (grid: the scratch sizing)
//   kNoBody, OverlapLds, stage_pair                                 x       x       x
//   stage_edge_dirs, edge_axis, edge_axis_of_table                  x       x       x
//   overlap_decide                                                  x               x
//   PassArgs, admit_record, for_each_held                           x       x       x
//   walk_cell_box                                                   x       x       x
//   kSweepReach                                                             x       x
//   spheres_overlap                                                                 x   (admit_record's reads once more)
//
// What a single family uses -- load_ray, may_reach, test_body, write_hit, wave_min; OverlapArgs; Sweep, load_sweep,
// sweep_may_reach, sweep_decide, SweepArgs; DistanceQ, load_distance, volume_desc, distance_decide, DistanceArgs -- is in its unit.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "xpbd_clip.hpp"
#include "xpbd_query.h"
#include "xpbd_query_shared.hpp"
#include "xpbd_pairs.h"
#include "xpbd_scan.h"
#include "xpbd_device.hpp"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kBruteRays = 8;      // rays per workgroup of the brute-force path (their winners stay in registers)
constexpr uint32_t kBruteBlocks = 2048; // the brute-force path splits the bodies until about this many workgroups run
// Cell edge = 2 * largest radius * kEdgeScale and every sphere's box is padded by largest radius * kPadScale before it is
// binned: a padded box is still narrower than a cell (at most 2 x 2 x 2 cells per body), and a body whose surface touches a
// cell face -- a hit point on the face, a ray running inside the face -- is listed in the cells on BOTH sides of it.  The DDA
// below locates points by rounded divisions; the pad (5e-8 of a cell) is far above their error as long as cell coordinates
// stay below kMaxCell (2^24 * 2^-52 = 2^-28 of a cell), and worlds whose box does not fit fall back to brute force per ray.
constexpr double kEdgeScale = 1.0 + 1e-6;
constexpr double kPadScale = 1e-7;
constexpr double kMaxCell = 16777216.0;   // |cell coordinate| <= 2^24
constexpr double kMaxDim = 1048576.0;     // cells per axis <= 2^20

struct QueryGrid {
    double edge, pad;
    int32_t lo[3];    // cell coordinates of the box of all padded spheres
    uint32_t dims[3];
    uint32_t mode;    // kEmpty, kGrid or kEveryBody
    uint32_t dense;   // key = linear cell index (else hashed)
    uint32_t mask;    // table_size - 1
};
constexpr uint32_t kEmpty = 0, kGrid = 1, kEveryBody = 2;

// A candidate of the winner: t, the index it is known by, the face, and the slot of its record.
struct Best {
    double t;
    uint32_t id, face, slot, pad;
};
static_assert(sizeof(Best) == 24, "brute-force partials are 24 bytes");

__device__ __forceinline__ bool better(double t, uint32_t id, const Best &b) { return t < b.t || (t == b.t && id < b.id); }

__device__ __forceinline__ Best no_hit() { return Best{INFINITY, XPBD_NO_HIT, XPBD_NO_HIT, XPBD_NO_HIT, 0}; }

__device__ __forceinline__ BodyQ load_body(const double *__restrict__ rec, uint32_t i)
{
    const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kQueryRecDoubles);
    const double2 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4], f = r[5];
    return BodyQ{Vec3{a.x, a.y, b.x}, Quat{b.y, c.x, c.y, d.x}, Vec3{d.y, e.x, e.y}, f.x};
}

__device__ __forceinline__ uint32_t query_key(const QueryGrid &g, int32_t x, int32_t y, int32_t z)
{
    if (g.dense)
        return (uint32_t)(x - g.lo[0]) + g.dims[0] * ((uint32_t)(y - g.lo[1]) + g.dims[1] * (uint32_t)(z - g.lo[2]));
    return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u)) & g.mask;
}

__device__ __forceinline__ int32_t clamp_axis(const QueryGrid &g, int a, double q)
{
    const double lo = (double)g.lo[a], hi = (double)g.lo[a] + (double)(g.dims[a] - 1u);
    q = q < lo ? lo : q; // (q is finite: the sphere is, and the grid's box holds it)
    return (int32_t)(q > hi ? hi : q);
}

// ---- the line walk shared by the rays and the sweeps' centre lines ------------------------------------------------------------
// Clip the line o + t * d, t in [0, tmax], to the grid's box grown by `grow` on every side: [t_near, t_far]; false: the line
// misses the box.  A ray passes grow = 0.0 and gets the plain box, bit for bit: x - 0.0 is x for every x, and hi + 0.0 differs
// from hi only for hi = -0.0, which (double)(a sum of integers) * edge cannot produce (such a sum is never -0.0, edge > 0).
__device__ __forceinline__ bool clip_to_grid(const QueryGrid &g, const double (&o)[3], const double (&d)[3], double tmax, double grow,
                                             double &t_near, double &t_far)
{
    t_near = 0.0, t_far = tmax;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)g.lo[a] * g.edge - grow, hi = ((double)g.lo[a] + (double)g.dims[a]) * g.edge + grow;
        if (d[a] == 0.0) {
            inside = inside && o[a] >= lo && o[a] <= hi;
        } else {
            const double t1 = (lo - o[a]) / d[a], t2 = (hi - o[a]) / d[a];
            const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
            t_near = tn > t_near ? tn : t_near;
            t_far = tf < t_far ? tf : t_far;
        }
    }
    return inside && t_near <= t_far;
}

// The axis of the nearest cell face ahead of `cell` and its t (-1 and +inf: the line does not move).  Each face's t comes from
// its own coordinate (no accumulated error); a line through an edge or a corner steps one axis at a time (first axis first),
// with equal t.
__device__ __forceinline__ int next_face(const QueryGrid &g, const int32_t (&cell)[3], const int32_t (&step)[3], const double (&o)[3],
                                         const double (&d)[3], double &t_next)
{
    double nearest = INFINITY; // (a local, not t_next, on purpose: a measured constraint, see DESIGN, "One walk, measured")
    int axis = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (step[a] != 0) {
            const double face = (double)(cell[a] + (step[a] > 0 ? 1 : 0)) * g.edge;
            const double ta = (face - o[a]) / d[a];
            if (ta < nearest) {
                nearest = ta;
                axis = a;
            }
        }
    t_next = nearest;
    return axis;
}

// ---- the group passes: overlap, sweep and distance queries --------------------------------------------------------------------
constexpr uint32_t kOverlapRecDoubles = 4; // per query: sphere centre xyz, radius (< 0: the query reports nothing)
constexpr uint32_t kNoBody = 0xFFFFFFFFu;

// Working set of one group: the world-space vertices of the volume (0, staged once per query) and of the candidate body (1),
// and each set in the other's local space; the world-space edge directions take the place of `local` for the edge axes.
template <uint32_t V>
struct OverlapLds {
    static constexpr uint32_t kVerts = V;
    double world[2][V][3];
    double local[2][V][3];
};

// Staging shared by the overlap and the sweep queries, for volume A (its world-space vertices already in s.world[0]) against body B
// by a group of 2 H lanes, `half` of which works for A (0) or B (1): A's vertices into B's local space, B's into world space and
// into A's local space -- vertices through their own frame into world space and through the inverse of the other frame.
template <class Lds>
__device__ __forceinline__ void stage_pair(Lds &s, const PolytopeTables &t, const ShapeDesc &da, const ShapeDesc &db, const Frame &fa_inv, const Frame &fb,
                                           const Frame &fb_inv, uint32_t half, uint32_t k, uint32_t H)
{
    __syncthreads(); // (one wave per workgroup: a fence; the previous candidate's reads are done)
    if (half == 0) {
        for (uint32_t vtx = k; vtx < da.n_verts; vtx += H)
            st3(s.local[0], vtx, fb_inv * ld3(s.world[0], vtx));
    } else {
        for (uint32_t vtx = k; vtx < db.n_verts; vtx += H) {
            const double *v = t.verts + 3 * (size_t)(db.vert0 + vtx);
            const Vec3 w = fb * Vec3{v[0], v[1], v[2]};
            st3(s.world[1], vtx, w);
            st3(s.local[1], vtx, fa_inv * w);
        }
    }
    __syncthreads();
}

// The world-space unique edge directions of both shapes into s.local (whose vertices the face queries are done with), when
// both tables fit it; false: edge_axis reads the tables.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool stage_edge_dirs(Lds &s, const PolytopeTables &t, const ShapeDesc &da, const ShapeDesc &db, const Frame &fa, const Frame &fb,
                                                uint32_t lane)
{
    const bool dirs_staged = da.n_dirs <= Lds::kVerts && db.n_dirs <= Lds::kVerts;
    __syncthreads();
    if (dirs_staged) {
        for (uint32_t d = lane; d < da.n_dirs + db.n_dirs; d += L) {
            const bool of_b = d >= da.n_dirs;
            const uint32_t kd = of_b ? d - da.n_dirs : d;
            const double *dd = t.edge_dirs + 3 * (size_t)((of_b ? db.dir0 : da.dir0) + kd);
            st3(s.local[of_b ? 1 : 0], kd, (of_b ? fb : fa).rotation * Vec3{dd[0], dd[1], dd[2]});
        }
        __syncthreads();
    }
    return dirs_staged;
}

// The axis of edge directions i of A and j of B; a component that is not finite means parallel directions: no axis.
__device__ __forceinline__ Vec3 edge_axis_of_table(const PolytopeTables &t, const ShapeDesc &da, const ShapeDesc &db, const Frame &fa, const Frame &fb,
                                                   uint32_t i, uint32_t j)
{
    const double *da_ = t.edge_dirs + 3 * (size_t)(da.dir0 + i), *db_ = t.edge_dirs + 3 * (size_t)(db.dir0 + j);
    return normalized(cross(fa.rotation * Vec3{da_[0], da_[1], da_[2]}, fb.rotation * Vec3{db_[0], db_[1], db_[2]}));
}

template <class Lds>
__device__ __forceinline__ Vec3 edge_axis(const Lds &s, bool dirs_staged, const PolytopeTables &t, const ShapeDesc &da, const ShapeDesc &db, const Frame &fa,
                                          const Frame &fb, uint32_t i, uint32_t j)
{
    return dirs_staged ? normalized(cross(ld3(s.local[0], i), ld3(s.local[1], j))) : edge_axis_of_table(t, da, db, fa, fb, i, j);
}

// The decision part of the SAT for volume A (frame fa, shape sa, its world-space vertices already in s.world[0]) against body
// B, by a group of L lanes: op_sat of the oracle up to its feature choice, with the arithmetic of the contact pipeline's
// sat_pair (xpbd_pairs.hip) -- vertices through their own frame into world space and through the inverse of the other frame
// into its local space, supports as LAST maxima under the total order, faces and edge-direction pairs as FIRST maxima.  True:
// not separated, with the feature and its separation.  Every lane of the group returns the same values.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool overlap_decide(Lds &s, const PolytopeTables &t, const Frame &fa, const Frame &fa_inv, uint32_t sa, const Frame &fb,
                                               uint32_t sb, uint32_t lane, uint32_t &feature, double &separation)
{
    constexpr uint32_t H = L / 2;
    const ShapeDesc da = t.desc[sa], db = t.desc[sb];
    if (da.n_verts == 0 || db.n_verts == 0 || da.n_faces == 0 || db.n_faces == 0)
        return false;
    const Frame fb_inv = inverse(fb);
    const uint32_t half = lane / H, k = lane % H; // first half of the group works for A, second for B
    stage_pair(s, t, da, db, fa_inv, fb, fb_inv, half, k, H);

    // ---- face queries: A's faces on the first half, B's on the second --------------------------------------------------
    double fdist = -DBL_MAX;
    uint32_t fidx = kNoBody;
    {
        const ShapeDesc dm = half ? db : da;
        const uint32_t n_other = half ? da.n_verts : db.n_verts;
        for (uint32_t f = k; f < dm.n_faces; f += H) {
            const double *pl = t.planes + 4 * (size_t)(dm.face0 + f);
            const Vec3 n{pl[0], pl[1], pl[2]}, dir = -n;
            Vec3 sup = ld3(s.local[half ^ 1u], 0);
            long long sup_key = total_key(dot(sup, dir));
            for (uint32_t v = 1; v < n_other; ++v) {
                const Vec3 x = ld3(s.local[half ^ 1u], v);
                const long long key = total_key(dot(x, dir));
                if (sup_key <= key) {
                    sup_key = key;
                    sup = x;
                }
            }
            const double dist = dot(n, sup) - pl[3];
            if (dist > fdist) { // ascending f on this lane: first maximum; a NaN never wins
                fdist = dist;
                fidx = f;
            }
        }
    }
    reduce_max_first(fdist, fidx, H);
    const double fdist_other = partner(fdist, H);
    const uint32_t fidx_other = partner(fidx, H);
    const double qa = half ? fdist_other : fdist, qb = half ? fdist : fdist_other;
    const uint32_t face_a = half ? fidx_other : fidx, face_b = half ? fidx : fidx_other;
    if (qa >= 0.0 || qb >= 0.0 || face_a == kNoBody || face_b == kNoBody)
        return false;

    // ---- edge axes: (unique edge direction of A) x (unique edge direction of B) -----------------------------------------
    double ebest = -DBL_MAX;
    uint32_t eq = kNoBody;
    const double *cca = t.centroids + 3 * (size_t)sa, *ccb = t.centroids + 3 * (size_t)sb;
    const Vec3 a_to_b = fb * Vec3{ccb[0], ccb[1], ccb[2]} - fa * Vec3{cca[0], cca[1], cca[2]};
    const bool dirs_staged = stage_edge_dirs<L>(s, t, da, db, fa, fb, lane);
    const uint32_t total = da.n_dirs * db.n_dirs;
    for (uint32_t q = lane; q < total; q += L) {
        const uint32_t i = q / db.n_dirs, j = q - i * db.n_dirs;
        Vec3 n = edge_axis(s, dirs_staged, t, da, db, fa, fb, i, j);
        if (!(fabs(n.x) <= DBL_MAX && fabs(n.y) <= DBL_MAX && fabs(n.z) <= DBL_MAX))
            continue; // parallel directions: a NaN axis contributes nothing
        if (dot(n, a_to_b) < 0.0)
            n = -n;
        double reach_a = dot(ld3(s.world[0], 0), n), reach_b = dot(ld3(s.world[1], 0), n);
        for (uint32_t v = 1; v < da.n_verts; ++v) {
            const double rr = dot(ld3(s.world[0], v), n);
            if (rr > reach_a)
                reach_a = rr;
        }
        for (uint32_t v = 1; v < db.n_verts; ++v) {
            const double rr = dot(ld3(s.world[1], v), n);
            if (rr < reach_b)
                reach_b = rr;
        }
        const double dist = reach_b - reach_a;
        if (dist > ebest) { // ascending q on this lane: first maximum
            ebest = dist;
            eq = q;
        }
    }
    reduce_max_first(ebest, eq, L);
    if (ebest >= 0.0)
        return false;
    const double face_best = qa > qb ? qa : qb;
    const bool use_edges = eq != kNoBody && ebest > face_best + kEdgeBias;
    feature = use_edges ? XPBD_FEATURE_EDGES : (qa == face_best ? XPBD_FEATURE_FACE_A : XPBD_FEATURE_FACE_B);
    separation = use_edges ? ebest : face_best;
    return true;
}

// What the overlap pass and the sweep pass are both given (n: queries or sweeps).
struct PassArgs {
    const double *qrec;         // k_overlap_queries or k_sweep_queries
    const double *rec;          // k_query_bodies
    const uint32_t *gid;        // the index a body is known by (null: its slot); XPBD_NO_HIT bodies have radius < 0 in rec
    const uint2 *filter;        // collision filters (null: every body in group ~0u)
    const QueryGrid *grid;      // grid path only
    const uint32_t *cell_start;
    const uint32_t *items;
    uint32_t n, masked, brute;
};

// The part of a candidate's admission that reads its record alone (one lane): a body that can be hit at all, not the one to
// ignore, in a group of the mask.  Its bounding sphere comes back for the caller's own last test.
__device__ __forceinline__ bool admit_record(const PassArgs &a, uint32_t i, uint32_t ignore, uint32_t mask, Vec3 &centre, double &radius)
{
    const double2 *r = reinterpret_cast<const double2 *>(a.rec + (size_t)i * kQueryRecDoubles);
    const double2 d = r[3], e = r[4], f = r[5];
    centre = Vec3{d.y, e.x, e.y};
    radius = f.x;
    if (!(radius >= 0.0))
        return false;
    if ((a.gid ? a.gid[i] : i) == ignore)
        return false;
    return !(a.masked && ((a.filter ? a.filter[i].x : ~0u) & mask) == 0);
}

// each(i), by the whole group, for every body the lanes of the group hold in `mine` (kNoBody: none), in lane order.
template <uint32_t L, class Each>
__device__ __forceinline__ void for_each_held(uint32_t mine, Each &&each)
{
    uint64_t todo = group_bits<L>(__ballot(mine != kNoBody));
    while (todo) {
        const uint32_t src = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1;
        each((uint32_t)__shfl((int)mine, (int)src, L));
    }
}

// The bodies listed in the box of cells qlo .. qlo + qdim - 1, each once: lane `lane` of a group of L takes cells lane, lane + L,
// ... of the box, admits the bodies listed there -- admit(i, centre, radius), one lane -- and whenever every lane holds a survivor
// or has run out of cells the group calls decide(mine).  seen(axis, lo, hi) is asked about the body's cell range on every axis:
// true on all three drops the body (the sweeps' "the previous stretch's box met it").
template <uint32_t L, class Admit, class Seen, class Decide>
__device__ __forceinline__ void walk_cell_box(const QueryGrid &g, const int32_t (&qlo)[3], const uint32_t (&qdim)[3], const uint32_t *cell_start,
                                              const uint32_t *items, uint32_t lane, Admit &&admit, Seen &&seen, Decide &&decide)
{
    const uint32_t cells = qdim[0] * qdim[1] * qdim[2];
    uint32_t next = lane, at = 0, end = 0, first = 0;
    int32_t cell[3] = {0, 0, 0};
    for (;;) {
        uint32_t mine = kNoBody;
        while (mine == kNoBody) {
            if (at == end) { // this lane's next cell
                if (next >= cells)
                    break;
                const uint32_t zy = next / qdim[0];
                cell[0] = qlo[0] + (int32_t)(next - zy * qdim[0]);
                cell[1] = qlo[1] + (int32_t)(zy % qdim[1]);
                cell[2] = qlo[2] + (int32_t)(zy / qdim[1]);
                next += L;
                const uint32_t key = query_key(g, cell[0], cell[1], cell[2]);
                first = at = cell_start[key];
                end = cell_start[key + 1];
                continue;
            }
            const uint32_t slot = at++, i = items[slot];
            Vec3 cb;
            double rb;
            if (!admit(i, cb, rb))
                continue;
            // A body is listed in up to 8 cells and the box covers several: the pair counts in ONE cell, the component-wise
            // maximum of the lower corners of the two cell ranges (k_query_bin's expressions).  A hashed key is shared by
            // several cells: the body must really be listed in this one, and once.
            const double c[3] = {cb.x, cb.y, cb.z};
            bool here = true, before = true;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const int32_t lo = clamp_axis(g, ax, floor((c[ax] - rb - g.pad) / g.edge));
                int32_t hi = clamp_axis(g, ax, floor((c[ax] + rb + g.pad) / g.edge));
                hi = hi > lo + 1 ? lo + 1 : hi;
                here = here && cell[ax] == (lo > qlo[ax] ? lo : qlo[ax]) && cell[ax] <= hi;
                before = before && seen(ax, lo, hi);
            }
            here = here && !before;
            if (here && !g.dense)
                for (uint32_t e = first; e < slot; ++e)
                    here = here && items[e] != i;
            if (here)
                mine = i;
        }
        if (!group_bits<L>(__ballot(mine != kNoBody)))
            break; // every lane has run out of cells
        decide(mine);
    }
}

constexpr double kSweepReach = 4.0;   // volumes wider than this many cell edges look at every body instead of walking cells

// The tight spheres of the overlap query's rule 2, with the body's sphere from its record.
__device__ __forceinline__ bool spheres_overlap(const double *__restrict__ rec, uint32_t i, Vec3 cq, double rq)
{
    const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kQueryRecDoubles);
    const double2 d = r[3], e = r[4], f = r[5];
    const Vec3 between = Vec3{d.y, e.x, e.y} - cq;
    const double reach = rq + f.x;
    return dot(between, between) < reach * reach;
}

} // namespace

} // namespace xpbd
