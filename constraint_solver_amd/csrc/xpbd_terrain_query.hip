// xpbd_terrain_query.hip -- the heightfield terrain in the scene queries (EXTENSION) for gfx950: the passes that put the terrain's
// answer next to the bodies' answer of a ray cast, a sweep and an overlap query (XPBD_QUERY_TERRAIN).
//
// Semantics: include/xpbd.h, "Terrain in the scene queries".  The terrain is the union of the prisms under its triangles; a
// ray's answer is the minimum over all triangles under (t, triangle).  A triangle's t is a function of the ray and the triangle
// alone, and neighbouring prisms compute the t of their shared wall and diagonal from the same expression, so the walk below
// -- which only chooses which cells are looked at -- cannot change a bit of the answer.  Nothing here writes anything but the
// callers' result arrays: no atomics, no scratch memory of its own (the distance pass stages the volume's vertices in LDS).
// The distance pass (xpbd_world_terrain_distance) is a call of its own, not a flag: see "distances" below.
#include <cmath>
#include <cstdint>

#include "xpbd_query.h"
#include "xpbd_query_shared.hpp"
#include "xpbd_step.hpp"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSweepLanes = 32; // lanes per sweep: one per vertex of the volume (XPBD_MAX_SHAPE_VERTS)
constexpr uint32_t kNoTriangle = 0xFFFFFFFFu;
static_assert(XPBD_MAX_SHAPE_VERTS <= kSweepLanes, "one lane per vertex of a swept volume");
static_assert(XPBD_HIT_TERRAIN < XPBD_NO_HIT, "a terrain hit wins a tie against a miss, and loses one against every body");

uint32_t blocks_of(uint32_t n, uint32_t per_block = kBlock) { return (n + per_block - 1) / per_block; }

// (The routines up to terrain_cast are host code too: a CPU build runs the walk against the brute-force minimum.)
struct Line {
    Vec3 o, d;
    double tmax;
};

// The terrain's answer so far: the minimum under (t, triangle); tri == kNoTriangle: nothing hit.
struct TerrainBest {
    double t;
    uint32_t tri;
};

// (isfinite by the name each side of the compilation knows it under: the distance walk's CPU check calls these on the host)
XPBD_HD bool finite1(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return isfinite(x);
#else
    return std::isfinite(x);
#endif
}
XPBD_HD bool finite3(Vec3 v) { return finite1(v.x) && finite1(v.y) && finite1(v.z); }

// The interval of one constraint list: the header's (s, v) rule and the slab rule of clip_to_grid (xpbd_query.hip).
struct Interval {
    double t_lo, t_hi;
    bool miss;

    XPBD_HD void plane(double s, double v)
    {
        if (s != s || v != v) {
            miss = true;
        } else if (v < 0.0) {
            const double tk = (-s) / v;
            if (tk > t_lo)
                t_lo = tk;
        } else if (v > 0.0) {
            const double tk = (-s) / v;
            t_hi = tk < t_hi ? tk : t_hi;
        } else if (s > 0.0) {
            miss = true;
        }
    }
    XPBD_HD void slab(double lo, double hi, double o, double d)
    {
        if (d == 0.0) {
            miss = miss || !(o >= lo && o <= hi);
        } else {
            const double t1 = (lo - o) / d, t2 = (hi - o) / d;
            const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
            t_lo = tn > t_lo ? tn : t_lo;
            t_hi = tf < t_hi ? tf : t_hi;
        }
    }
};

// Both triangles of cell (i, j) against the line: one 64-byte record.
XPBD_HD void test_cell(const Terrain &tr, uint32_t i, uint32_t j, const Line &r, TerrainBest &best)
{
    const uint32_t cell = j * (tr.nx - 1) + i;
    const double2 *rec = reinterpret_cast<const double2 *>(tr.planes + (size_t)cell * 8);
    const double2 a = rec[0], b = rec[1], c = rec[2], e = rec[3];
    const double xi = tr.x0 + (double)i * tr.dx, xi1 = tr.x0 + (double)(i + 1) * tr.dx;
    const double yj = tr.y0 + (double)j * tr.dy, yj1 = tr.y0 + (double)(j + 1) * tr.dy;
    const double g = (r.o.x - xi) * tr.dy - (r.o.y - yj) * tr.dx, gv = r.d.x * tr.dy - r.d.y * tr.dx;
#pragma unroll
    for (uint32_t upper = 0; upper < 2; ++upper) {
        const Plane pl = upper ? Plane{Vec3{c.x, c.y, e.x}, e.y} : Plane{Vec3{a.x, a.y, b.x}, b.y};
        Interval iv{0.0, r.tmax, false};
        iv.plane(distance(pl, r.o), dot(pl.normal, r.d));
        iv.slab(xi, xi1, r.o.x, r.d.x);
        iv.slab(yj, yj1, r.o.y, r.d.y);
        iv.plane(upper ? g : -g, upper ? gv : -gv);
        const uint32_t tri = 2u * cell + upper;
        if (!iv.miss && iv.t_lo <= iv.t_hi && (iv.t_lo < best.t || (iv.t_lo == best.t && tri < best.tri)))
            best = TerrainBest{iv.t_lo, tri};
    }
}

// One axis of the walk.  The nc cells of the axis are numbered by POSITION p along the line's direction (p = the cell's index
// when the line moves up the axis, nc - 1 - index when it moves down); position p lies between the borders q = p and q = p + 1,
// and key(q) -- the slab expression of the border itself, (border - o) / d, never accumulated -- does not decrease with q.  The
// cells whose closed interval [key(p), key(p + 1)] holds the current t are the range lo .. hi.  An axis the line does not move
// along takes the border's coordinate as its key and the origin's coordinate in place of t: its range never changes.
struct WalkAxis {
    double c0, dc, o, d;
    uint32_t nc, lo, hi;
    bool moving, forward;
    double ahead;

    XPBD_HD double key(uint32_t q) const
    {
        const double border = c0 + (double)(forward ? q : nc - q) * dc;
        return moving ? (border - o) / d : border;
    }
    XPBD_HD uint32_t index_of(uint32_t p) const { return forward ? p : nc - 1u - p; }
    // hi = the last position whose near border is not beyond tau (searched upwards from `from`, then downwards), lo = the
    // first whose far border is not before it.
    XPBD_HD void settle(double tau, uint32_t from)
    {
        uint32_t p = from;
        while (p + 1u < nc && key(p + 1u) <= tau)
            ++p;
        while (p > 0u && key(p) > tau)
            --p;
        hi = p;
        while (p > 0u && key(p) >= tau)
            --p;
        lo = p;
    }
    // The ranges at the first t of the walk, after an estimate from floor; false: no cell of the axis holds tau.
    XPBD_HD bool start(double tau, double t)
    {
        if (!(key(0u) <= tau && tau <= key(nc)))
            return false;
        const double u = ((moving ? o + t * d : o) - c0) / dc;
        const double top = (double)(nc - 1u);
        const uint32_t cell = u >= 0.0 ? (u < top ? (uint32_t)floor(u) : nc - 1u) : 0u; // (a NaN: cell 0)
        settle(tau, index_of(cell));
        ahead = last() ? INFINITY : key(hi + 1u);
        return true;
    }
    // Whether the range has reached the axis's last cell for good; `ahead` is when the line crosses the next border beyond the
    // range (+inf: there is none).
    XPBD_HD bool last() const { return !moving || hi + 1u >= nc; }
    // The range at a later t, the smaller of the two axes' `ahead`.  key(hi) is at most the previous t, so below this one: every
    // cell behind hi has ended.  If this axis is the one that crosses (ahead == t), cell hi ends exactly now and stays as lo, and
    // the range runs on through every cell that also begins at t: one division per border crossed, none otherwise.  The loop is
    // bounded by the axis itself, not by `ahead`: a border's t overflows to +inf when the direction component is tiny, t can
    // then be +inf as well, and +inf <= +inf holds for the "none" value too.
    XPBD_HD void advance(double t)
    {
        lo = hi;
        while (hi + 1u < nc && ahead <= t) {
            ++hi;
            ahead = last() ? INFINITY : key(hi + 1u);
        }
    }
};

// The terrain's answer for one line, no later than `bound` (a hit the caller already has: a later one cannot win).
template <bool BRUTE>
XPBD_HD TerrainBest terrain_cast(const Terrain &tr, const Line &r, double bound)
{
    TerrainBest best{INFINITY, kNoTriangle};
    const uint32_t cx = tr.nx - 1u, cy = tr.ny - 1u;
    if (BRUTE) {
        for (uint32_t j = 0; j < cy; ++j)
            for (uint32_t i = 0; i < cx; ++i)
                test_cell(tr, i, j, r, best);
        return best;
    }
    WalkAxis ax{tr.x0, tr.dx, r.o.x, r.d.x, cx, 0u, 0u, r.d.x != 0.0, !(r.d.x < 0.0)};
    WalkAxis ay{tr.y0, tr.dy, r.o.y, r.d.y, cy, 0u, 0u, r.d.y != 0.0, !(r.d.y < 0.0)};
    // the line clipped to the field's box: no prism is hit outside [t, t_end]
    double t = 0.0, t_end = r.tmax;
    if (ax.moving) {
        const double tn = ax.key(0u), tf = ax.key(cx);
        t = tn > t ? tn : t;
        t_end = tf < t_end ? tf : t_end;
    }
    if (ay.moving) {
        const double tn = ay.key(0u), tf = ay.key(cy);
        t = tn > t ? tn : t;
        t_end = tf < t_end ? tf : t_end;
    }
    if (!(t <= t_end) || !ax.start(ax.moving ? t : r.o.x, t) || !ay.start(ay.moving ? t : r.o.y, t))
        return best;
    // the previous rectangle (none yet: empty), whose cells have been looked at
    uint32_t pxl = 1u, pxh = 0u, pyl = 1u, pyh = 0u;
    for (;;) {
        if (t > bound || t > best.t) // strict: a cell that begins at the best t can still win on the smaller triangle
            break;
        for (uint32_t py = ay.lo; py <= ay.hi; ++py)
            for (uint32_t px = ax.lo; px <= ax.hi; ++px)
                if (!(px >= pxl && px <= pxh && py >= pyl && py <= pyh))
                    test_cell(tr, ax.index_of(px), ay.index_of(py), r, best);
        const double t_next = ax.ahead < ay.ahead ? ax.ahead : ay.ahead;
        // (else an axis moves on, at most cx + cy rounds: t_next is beyond t by the ranges' construction, and the explicit test
        // ends the walk should it ever not be -- after a round at t = +inf, say)
        if ((ax.last() && ay.last()) || !(t_next <= t_end) || !(t_next > t))
            break;
        pxl = ax.lo, pxh = ax.hi, pyl = ay.lo, pyh = ay.hi;
        t = t_next;
        if (ax.moving)
            ax.advance(t);
        if (ay.moving)
            ay.advance(t);
    }
    return best;
}

// ---- rays: after the body pass, one lane per ray -----------------------------------------------------------------------------
template <bool BRUTE>
__global__ void __launch_bounds__(kBlock) k_terrain_rays(Terrain tr, const xpbd_ray *__restrict__ rays, uint32_t n_rays, xpbd_ray_hit *__restrict__ hits)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays)
        return;
    const xpbd_ray &x = rays[r];
    const Line line{Vec3{x.origin[0], x.origin[1], x.origin[2]}, Vec3{x.direction[0], x.direction[1], x.direction[2]}, x.max_distance};
    const bool moving = line.d.x != 0.0 || line.d.y != 0.0 || line.d.z != 0.0;
    if (!(finite3(line.o) && finite3(line.d) && moving && line.tmax >= 0.0)) // (the body pass's rule: such a ray hits nothing)
        return;
    const uint32_t body = hits[r].body;
    const double distance = hits[r].distance; // +inf after a miss
    const TerrainBest best = terrain_cast<BRUTE>(tr, line, distance);
    if (best.tri == kNoTriangle)
        return;
    if (!(best.t < distance || (best.t == distance && XPBD_HIT_TERRAIN < body))) // the order (t, body): a body wins a tie
        return;
    xpbd_ray_hit h;
    h.body = XPBD_HIT_TERRAIN;
    h.distance = best.t;
    const Vec3 p = line.o + line.d * best.t;
    h.point[0] = p.x, h.point[1] = p.y, h.point[2] = p.z;
    if (best.t > 0.0) { // something entered
        const double *pl = tr.planes + (size_t)best.tri * 4;
        h.face = best.tri;
        h.normal[0] = pl[0], h.normal[1] = pl[1], h.normal[2] = pl[2];
    } else {
        h.face = XPBD_RAY_INSIDE;
        h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    }
    hits[r] = h;
}

// ---- sweeps: after k_sweep_pass, one group of kSweepLanes lanes per sweep, one lane per vertex of the volume ------------------
template <bool BRUTE>
__global__ void __launch_bounds__(kBlock) k_terrain_sweeps(Terrain tr, PolytopeTables t, const xpbd_sweep *__restrict__ sweeps, uint32_t n_sweeps,
                                                           const double *__restrict__ qrec, xpbd_sweep_hit *__restrict__ hits)
{
    const uint32_t q = blockIdx.x * (kBlock / kSweepLanes) + threadIdx.x / kSweepLanes, lane = threadIdx.x % kSweepLanes;
    if (q >= n_sweeps)
        return;
    TerrainBest best{INFINITY, kNoTriangle};
    uint32_t vertex = kNoTriangle;
    const xpbd_sweep &x = sweeps[q];
    const Vec3 d{x.direction[0], x.direction[1], x.direction[2]};
    const Vec3 position{x.position[0], x.position[1], x.position[2]};
    const double distance = hits[q].distance;
    if (qrec[(size_t)q * 4 + 3] >= 0.0) { // k_sweep_queries: the sweep can hit something
        const Frame fa{position, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
        const ShapeDesc da = t.desc[x.shape];
        for (uint32_t v = lane; v < da.n_verts; v += kSweepLanes) {
            const double *a = t.verts + 3 * (size_t)(da.vert0 + v);
            const Line line{fa * Vec3{a[0], a[1], a[2]}, d, x.max_distance};
            if (!finite3(line.o))
                continue;
            const TerrainBest b = terrain_cast<BRUTE>(tr, line, distance);
            if (b.tri != kNoTriangle && (b.t < best.t || (b.t == best.t && b.tri < best.tri))) { // ascending v: the first vertex stays
                best = b;
                vertex = v;
            }
        }
    }
    for (uint32_t off = kSweepLanes >> 1; off; off >>= 1) {
        const double ot = __shfl_xor(best.t, off, kSweepLanes);
        const uint32_t otri = __shfl_xor(best.tri, off, kSweepLanes), ov = __shfl_xor(vertex, off, kSweepLanes);
        if (otri != kNoTriangle && (ot < best.t || (ot == best.t && (otri < best.tri || (otri == best.tri && ov < vertex))))) {
            best = TerrainBest{ot, otri};
            vertex = ov;
        }
    }
    if (lane != 0 || best.tri == kNoTriangle || !(best.t < distance)) // strictly earlier than the body's hit
        return;
    xpbd_sweep_hit h;
    h.body = XPBD_HIT_TERRAIN;
    h.reserved = 0;
    h.distance = best.t;
    const Vec3 p = position + d * best.t;
    h.position[0] = p.x, h.position[1] = p.y, h.position[2] = p.z;
    if (best.t > 0.0) {
        const double *pl = tr.planes + (size_t)best.tri * 4;
        h.feature = XPBD_FEATURE_FACE_B;
        h.face = best.tri;
        h.normal[0] = pl[0], h.normal[1] = pl[1], h.normal[2] = pl[2];
    } else { // a vertex starts in or under the ground
        h.feature = XPBD_SWEEP_INITIAL;
        h.face = XPBD_NO_HIT;
        h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    }
    hits[q] = h;
}

// ---- overlaps: one lane per query, the stepper's own lookup at every vertex of the volume ----------------------------------------
// FILL = false, between the count pass and the scan: a volume with a vertex under the ground counts one entry more.
// FILL = true, after the fill pass and before the sort: that entry, the last of the query's segment (its index is the largest).
template <bool FILL>
__global__ void __launch_bounds__(kBlock) k_terrain_overlap(Terrain tr, PolytopeTables t, const xpbd_overlap_query *__restrict__ queries, uint32_t n_queries,
                                                            const double *__restrict__ qrec, uint32_t *__restrict__ offsets,
                                                            xpbd_overlap_hit *__restrict__ hits, uint32_t cap)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries || !(qrec[(size_t)q * 4 + 3] >= 0.0)) // k_overlap_queries: the query can report something
        return;
    const xpbd_overlap_query &x = queries[q];
    const Frame fq{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
    const ShapeDesc dq = t.desc[x.shape];
    bool touches = false;
    double lowest = 0.0;
    for (uint32_t v = 0; v < dq.n_verts; ++v) {
        const double *a = t.verts + 3 * (size_t)(dq.vert0 + v);
        const Vec3 p = fq * Vec3{a[0], a[1], a[2]};
        Plane plane;
        if (!terrain_plane(tr, p, plane))
            continue;
        const double s = distance(plane, p);
        if (s < 0.0 && (!touches || s < lowest)) { // the first minimum
            touches = true;
            lowest = s;
        }
    }
    if (!touches)
        return;
    if (!FILL) {
        offsets[q] += 1u;
        return;
    }
    const uint32_t slot = offsets[q + 1] - 1u;
    if (slot < cap) {
        xpbd_overlap_hit h;
        h.body = XPBD_HIT_TERRAIN;
        h.feature = XPBD_FEATURE_FACE_B;
        h.separation = lowest;
        hits[slot] = h;
    }
}

// ---- distances: the terrain feature nearest to a convex volume or a point ---------------------------------------------------------
// Semantics: include/xpbd.h, "Terrain in the distance queries".  The answer is the minimum over ALL features of the surface under
// the total order (d2, class, terrain feature number, volume index); a candidate's d2 is a function of the query and the feature
// alone, and every feature has one number and one owner -- sample (i, j) owns the two triangles of cell (i, j), itself, and the
// three edges that start at it -- so the walk below, which only chooses the samples, cannot change a bit of the answer.
// (The routines up to terrain_distance_walk and terrain_distance_record are host code too: a CPU build runs the walk against the
// brute-force minimum.)
#ifndef XPBD_TERRAIN_DISTANCE_LANES
#define XPBD_TERRAIN_DISTANCE_LANES 8      // measured against 16, 32 and 64 ("Terrain in the distance queries"; a build flag for that A/B only)
#endif
constexpr uint32_t kDistanceLanes = XPBD_TERRAIN_DISTANCE_LANES; // lanes per query; the samples of a ring are shared out among them
static_assert(kDistanceLanes == 8 || kDistanceLanes == 16 || kDistanceLanes == 32 || kDistanceLanes == 64, "a group is a power-of-two part of a wave");
constexpr uint64_t kNoCandidate = ~0ull;   // DistanceBest::key before anything counted
constexpr double kNotSeparated = -1.0;     // DistanceBest::d2 of rule 1: below every squared distance, so it wins every minimum

// The minimum so far.  key = class << 56 | terrain feature number << 16 | the volume's index (vertex, face or edge): the number of
// a feature is below 2^24 (XPBD_MAX_TERRAIN_SAMPLES * 3), the volume's index below 2^16.
struct DistanceBest {
    double d2;
    uint64_t key;

    XPBD_HD void offer(double x, uint32_t cls, uint32_t feature, uint32_t index)
    {
        const uint64_t k = (uint64_t)cls << 56 | (uint64_t)feature << 16 | index;
        if (x < d2 || (x == d2 && key != kNoCandidate && k < key)) { // (a NaN never replaces; nor does +inf the empty minimum)
            d2 = x;
            key = k;
        }
    }
};
static_assert(3ull * XPBD_MAX_TERRAIN_SAMPLES <= (1ull << 24), "a terrain feature's number fits 24 bits of the key");

// The minimum over the L lanes of a group, left in every lane.  (A host build is a group of one lane.)
template <uint32_t L>
XPBD_HD void group_min(DistanceBest &b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t off = L >> 1; off; off >>= 1) {
        const double od = __shfl_xor(b.d2, off, L);
        const unsigned long long ok = __shfl_xor((unsigned long long)b.key, off, L);
        if (od < b.d2 || (od == b.d2 && ok < b.key))
            b = DistanceBest{od, ok};
    }
#else
    (void)b; // (a CPU program calls the walk with L = 1)
#endif
}

// The volume of one query as the candidates see it.
struct DistanceVolume {
    Frame fa, fa_inv;
    ShapeDesc da;   // the point volume: one vertex, no faces, one edge from it to itself
    uint32_t shape;
    bool point;
    Vec3 c;         // centre and radius of the bounding sphere, as k_distance_queries forms them
    double rs;
    double dmax;
    bool valid;     // the query can find something: a shape of the table or the point, a finite frame, a max_distance >= 0
};

XPBD_HD DistanceVolume load_distance_volume(const PolytopeTables &t, const xpbd_distance_query &x)
{
    DistanceVolume vol{};
    vol.fa = Frame{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
    vol.shape = x.shape;
    vol.point = x.shape == XPBD_DISTANCE_POINT;
    vol.dmax = x.max_distance;
    vol.c = Vec3{0.0, 0.0, 0.0};
    vol.rs = -1.0;
    vol.valid = false;
    if (vol.point || x.shape < t.n_shapes) {
        vol.da = vol.point ? ShapeDesc{0, 1, 0, 0, 0, 1, 0, 0} : t.desc[x.shape];
        vol.c = vol.fa.position;
        double rs = 0.0;
        if (!vol.point) {
            const double *cc = t.centroids + 3 * (size_t)x.shape;
            vol.c = vol.fa * Vec3{cc[0], cc[1], cc[2]};
            rs = t.radii[x.shape];
        }
        const bool finite = finite3(vol.fa.position) && finite1(vol.fa.rotation.s) && finite1(vol.fa.rotation.x) && finite1(vol.fa.rotation.y) &&
                            finite1(vol.fa.rotation.z) && finite3(vol.c);
        if (finite && vol.dmax >= 0.0 && rs >= 0.0 && vol.da.n_verts <= XPBD_MAX_SHAPE_VERTS) { // (a NaN max_distance fails; +inf passes)
            vol.rs = rs;
            vol.valid = true;
            vol.fa_inv = inverse(vol.fa);
        }
    }
    return vol;
}

// World vertex v of the volume: aw_v = fa * a_v; the point volume's is `position` itself.
XPBD_HD Vec3 volume_vertex(const PolytopeTables &t, const DistanceVolume &vol, uint32_t v)
{
    if (vol.point)
        return vol.fa.position;
    const double *a = t.verts + 3 * (size_t)(vol.da.vert0 + v);
    return vol.fa * Vec3{a[0], a[1], a[2]};
}

XPBD_HD void volume_edge(const PolytopeTables &t, const DistanceVolume &vol, uint32_t e, uint32_t &a0, uint32_t &a1)
{
    a0 = a1 = 0;
    if (!vol.point) {
        const uint32_t *ea = t.edges + 2 * (size_t)(vol.da.edge0 + e);
        a0 = ea[0], a1 = ea[1];
    }
}

XPBD_HD Vec3 terrain_sample(const TerrainHeights &tf, uint32_t i, uint32_t j)
{
    return Vec3{tf.tr.x0 + (double)i * tf.tr.dx, tf.tr.y0 + (double)j * tf.tr.dy, tf.heights[(size_t)j * tf.tr.nx + i]};
}

// The far end of terrain edge (i, j, e): 0 along x, 1 along y, 2 the diagonal.
XPBD_HD Vec3 terrain_edge_end(const TerrainHeights &tf, uint32_t i, uint32_t j, uint32_t e)
{
    return terrain_sample(tf, e == 1 ? i : i + 1, e == 0 ? j : j + 1);
}

// Rule 2 (a) for one vertex and one triangle: whether the candidate counts, with h and the foot.
XPBD_HD bool vertex_over_triangle(const Terrain &tr, uint32_t i, uint32_t j, uint32_t upper, const Plane &pl, Vec3 p, double &h, Vec3 &foot)
{
    h = dot(pl.normal, p) - pl.displacement;
    if (!(h >= 0.0))
        return false;
    foot = p - h * pl.normal;
    const double xi = tr.x0 + (double)i * tr.dx, xi1 = tr.x0 + (double)(i + 1) * tr.dx;
    const double yj = tr.y0 + (double)j * tr.dy, yj1 = tr.y0 + (double)(j + 1) * tr.dy;
    if (!(xi <= foot.x && foot.x <= xi1 && yj <= foot.y && foot.y <= yj1))
        return false;
    const double g = (foot.x - xi) * tr.dy - (foot.y - yj) * tr.dx;
    return upper ? g <= 0.0 : g >= 0.0;
}

XPBD_HD Plane triangle_plane(const Terrain &tr, uint32_t tri)
{
    const double *pl = tr.planes + (size_t)tri * 4;
    return Plane{Vec3{pl[0], pl[1], pl[2]}, pl[3]};
}

// Everything sample (i, j) owns against the volume: its two triangles (a), itself (b), its up to three edges (c) and rule 1 (ii).
// aw: the volume's world vertices.
XPBD_HD void distance_sample(const TerrainHeights &tf, const PolytopeTables &t, const DistanceVolume &vol, const Vec3 *aw, uint32_t i, uint32_t j,
                             DistanceBest &best)
{
    const Terrain &tr = tf.tr;
    const bool has_x = i + 1u < tr.nx, has_y = j + 1u < tr.ny;
    const uint32_t sample = j * tr.nx + i;
    if (has_x && has_y) { // (a)
        const uint32_t cell = j * (tr.nx - 1u) + i;
        for (uint32_t upper = 0; upper < 2; ++upper) {
            const uint32_t tri = 2u * cell + upper;
            const Plane pl = triangle_plane(tr, tri);
            for (uint32_t v = 0; v < vol.da.n_verts; ++v) {
                double h;
                Vec3 foot;
                if (vertex_over_triangle(tr, i, j, upper, pl, aw[v], h, foot))
                    best.offer(h * h, 0u, tri, v);
            }
        }
    }
    const Vec3 P = terrain_sample(tf, i, j);
    if (!vol.point) { // (b)
        const Vec3 p = vol.fa_inv * P;
        for (uint32_t f = 0; f < vol.da.n_faces; ++f) {
            double h;
            Vec3 foot;
            if (vertex_over_face(t, vol.da.vert0, vol.da.face0 + f, p, INFINITY, h, foot))
                best.offer(h * h, 1u, sample, f);
        }
    }
    for (uint32_t e = 0; e < 3; ++e) { // (c), and rule 1 (ii)
        if (!(e == 0 ? has_x : (e == 1 ? has_y : has_x && has_y)))
            continue;
        const Vec3 Q = terrain_edge_end(tf, i, j, e);
        if (!vol.point) {
            const Ray ray{P, Q - P, 1.0, XPBD_NO_HIT, true};
            const BodyQ q{vol.fa_inv.position, vol.fa_inv.rotation, vol.c, vol.rs};
            double t_hit;
            uint32_t face;
            if (ray_body(ray, q, t, vol.shape, t_hit, face))
                best = DistanceBest{kNotSeparated, 0ull};
        }
        for (uint32_t k = 0; k < vol.da.n_edges; ++k) {
            uint32_t a0, a1;
            volume_edge(t, vol, k, a0, a1);
            Vec3 ca, cb;
            best.offer(segment_closest(aw[a0], aw[a1], P, Q, ca, cb), 2u, 3u * sample + e, k);
        }
    }
}

// floor((c - c0) / dc) clamped into the samples 0 .. n - 1 (a NaN: 0).
XPBD_HD int32_t centre_sample(double c, double c0, double dc, uint32_t n)
{
    const double u = (c - c0) / dc, top = (double)(n - 1u);
    return u >= 0.0 ? (u < top ? (int32_t)floor(u) : (int32_t)(n - 1u)) : 0;
}

// The minimum of one query by a group of L lanes (lane = this one's number in it); every lane returns it.  best.d2 ==
// kNotSeparated: rule 1; best.key == kNoCandidate: nothing counted.  BRUTE: every sample.  Otherwise rings of samples around the
// one under the volume's centre.  Ring r >= 1 and all beyond it lie outside the open rectangle between the borders x(ci - r + 1),
// x(ci + r), y(cj - r + 1), y(cj + r) -- of those sides on which the field still has samples -- so once the bounding sphere is
// further inside than min(max_distance, best so far) from every such side, no ring can hold the minimum or a tie with it.  The
// test carries the conservative slack of the body pass; it is never part of the definition.  At most max(nx, ny) rings: a +inf
// query, a NaN bound and a volume beside the field end with the field.
template <bool BRUTE, uint32_t L>
XPBD_HD DistanceBest terrain_distance_walk(const TerrainHeights &tf, const PolytopeTables &t, const DistanceVolume &vol, const Vec3 *aw, uint32_t lane,
                                           uint32_t *looked_at = nullptr)
{
    const Terrain &tr = tf.tr;
    DistanceBest best{INFINITY, kNoCandidate};
    // rule 1 (i): a vertex under the plane of the stepper's lookup
    for (uint32_t v = lane; v < vol.da.n_verts; v += L) {
        Plane pl;
        if (terrain_plane(tr, aw[v], pl) && distance(pl, aw[v]) < 0.0)
            best = DistanceBest{kNotSeparated, 0ull};
    }
    group_min<L>(best);
    if (best.d2 < 0.0)
        return best;
    if (BRUTE) {
        const uint32_t samples = tr.nx * tr.ny;
        for (uint32_t s = lane; s < samples; s += L)
            distance_sample(tf, t, vol, aw, s % tr.nx, s / tr.nx, best);
        group_min<L>(best);
        return best;
    }
    const int32_t nx = (int32_t)tr.nx, ny = (int32_t)tr.ny;
    const int32_t ci = centre_sample(vol.c.x, tr.x0, tr.dx, tr.nx), cj = centre_sample(vol.c.y, tr.y0, tr.dy, tr.ny);
    const int32_t rings = nx > ny ? nx : ny;
    if (lane == 0)
        distance_sample(tf, t, vol, aw, (uint32_t)ci, (uint32_t)cj, best);
    if (looked_at)
        *looked_at += 1u;
    group_min<L>(best);
    for (int32_t r = 1; r < rings && !(best.d2 < 0.0); ++r) {
        const bool left = ci >= r, right = ci + r <= nx - 1, low = cj >= r, high = cj + r <= ny - 1;
        if (!(left || right || low || high))
            break;
        double g = INFINITY; // how far inside the nearest side the centre lies
        if (left) {
            const double s = vol.c.x - (tr.x0 + (double)(ci - r + 1) * tr.dx);
            g = s < g ? s : g;
        }
        if (right) {
            const double s = (tr.x0 + (double)(ci + r) * tr.dx) - vol.c.x;
            g = s < g ? s : g;
        }
        if (low) {
            const double s = vol.c.y - (tr.y0 + (double)(cj - r + 1) * tr.dy);
            g = s < g ? s : g;
        }
        if (high) {
            const double s = (tr.y0 + (double)(cj + r) * tr.dy) - vol.c.y;
            g = s < g ? s : g;
        }
        const double so_far = sqrt(best.d2), reach = vol.rs + (so_far < vol.dmax ? so_far : vol.dmax);
        if (g > 0.0 && g * g > reach * reach * kSphereSlack + 1e-12 * (g * g))
            break;
        // the ring inside the field: its two rows, then its two columns between them
        const int32_t ilo = left ? ci - r : 0, ihi = right ? ci + r : nx - 1;
        const int32_t jlo = low ? cj - r + 1 : 0, jhi = high ? cj + r - 1 : ny - 1;
        const int32_t row = ihi - ilo + 1, col = jhi >= jlo ? jhi - jlo + 1 : 0;
        const int32_t n0 = low ? row : 0, n1 = high ? row : 0, n2 = left ? col : 0, n3 = right ? col : 0;
        const int32_t total = n0 + n1 + n2 + n3;
        for (int32_t k = (int32_t)lane; k < total; k += (int32_t)L) {
            int32_t i, j;
            if (k < n0)
                i = ilo + k, j = cj - r;
            else if (k < n0 + n1)
                i = ilo + (k - n0), j = cj + r;
            else if (k < n0 + n1 + n2)
                i = ci - r, j = jlo + (k - n0 - n1);
            else
                i = ci + r, j = jlo + (k - n0 - n1 - n2);
            distance_sample(tf, t, vol, aw, (uint32_t)i, (uint32_t)j, best);
        }
        if (looked_at)
            *looked_at += (uint32_t)total;
        group_min<L>(best);
    }
    return best;
}

// The record of a query's minimum: the winning candidate once more, by the expressions that measured it.
XPBD_HD xpbd_distance_hit terrain_distance_record(const TerrainHeights &tf, const PolytopeTables &t, const DistanceVolume &vol, const Vec3 *aw,
                                                  const DistanceBest &best)
{
    xpbd_distance_hit h;
    h.body = XPBD_NO_HIT;
    h.feature = 0;
    h.index_a = h.index_b = XPBD_NO_HIT;
    h.distance = INFINITY;
    h.point_a[0] = h.point_a[1] = h.point_a[2] = 0.0;
    h.point_b[0] = h.point_b[1] = h.point_b[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (!vol.valid || best.key == kNoCandidate)
        return h;
    if (best.d2 < 0.0) {
        h.body = XPBD_HIT_TERRAIN;
        h.feature = XPBD_DISTANCE_OVERLAP;
        h.distance = 0.0;
        return h;
    }
    const double dist = sqrt(best.d2);
    if (!(dist <= vol.dmax))
        return h;
    const uint32_t cls = (uint32_t)(best.key >> 56), feature = (uint32_t)(best.key >> 16) & 0xFFFFFFu, index = (uint32_t)best.key & 0xFFFFu;
    const Terrain &tr = tf.tr;
    Vec3 pa{0.0, 0.0, 0.0}, pb{0.0, 0.0, 0.0};
    double hh = 0.0;
    if (cls == 0u) {
        const uint32_t cell = feature >> 1, j = cell / (tr.nx - 1u), i = cell - j * (tr.nx - 1u);
        pa = aw[index];
        vertex_over_triangle(tr, i, j, feature & 1u, triangle_plane(tr, feature), pa, hh, pb);
        h.feature = XPBD_FEATURE_FACE_B;
    } else if (cls == 1u) {
        const uint32_t j = feature / tr.nx, i = feature - j * tr.nx;
        Vec3 foot{0.0, 0.0, 0.0};
        pb = terrain_sample(tf, i, j);
        vertex_over_face(t, vol.da.vert0, vol.da.face0 + index, vol.fa_inv * pb, INFINITY, hh, foot);
        pa = vol.fa * foot;
        h.feature = XPBD_FEATURE_FACE_A;
    } else {
        const uint32_t sample = feature / 3u, e = feature - 3u * sample, j = sample / tr.nx, i = sample - j * tr.nx;
        uint32_t a0, a1;
        volume_edge(t, vol, index, a0, a1);
        segment_closest(aw[a0], aw[a1], terrain_sample(tf, i, j), terrain_edge_end(tf, i, j, e), pa, pb);
        h.feature = XPBD_FEATURE_EDGES;
    }
    h.body = XPBD_HIT_TERRAIN;
    h.index_a = index, h.index_b = feature;
    h.distance = dist;
    h.point_a[0] = pa.x, h.point_a[1] = pa.y, h.point_a[2] = pa.z;
    h.point_b[0] = pb.x, h.point_b[1] = pb.y, h.point_b[2] = pb.z;
    if (dist != 0.0) {
        const Vec3 n = (pa - pb) * (1.0 / dist);
        h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
    }
    return h;
}

// One group of L lanes per query; lane 0 writes the record.
template <bool BRUTE, uint32_t L>
__global__ void __launch_bounds__(kBlock) k_terrain_distance(TerrainHeights tf, PolytopeTables t, const xpbd_distance_query *__restrict__ queries,
                                                             uint32_t n_queries, xpbd_distance_hit *__restrict__ hits)
{
    constexpr uint32_t PB = kBlock / L;
    __shared__ Vec3 s_aw[PB][XPBD_MAX_SHAPE_VERTS];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PB + group;
    const bool live = q < n_queries;
    DistanceVolume vol{};
    if (live) {
        vol = load_distance_volume(t, queries[q]);
        if (vol.valid)
            for (uint32_t v = lane; v < vol.da.n_verts; v += L)
                s_aw[group][v] = volume_vertex(t, vol, v);
    }
    __syncthreads();
    if (!live)
        return;
    DistanceBest best{INFINITY, kNoCandidate};
    if (vol.valid)
        best = terrain_distance_walk<BRUTE, L>(tf, t, vol, s_aw[group], lane);
    if (lane == 0)
        hits[q] = terrain_distance_record(tf, t, vol, s_aw[group], best);
}

} // namespace

hipError_t launch_terrain_rays(const Terrain &terrain, const void *rays, uint32_t n_rays, bool brute, void *hits, hipStream_t stream)
{
    if (n_rays == 0)
        return hipSuccess;
    const xpbd_ray *r = static_cast<const xpbd_ray *>(rays);
    xpbd_ray_hit *h = static_cast<xpbd_ray_hit *>(hits);
    if (brute)
        hipLaunchKernelGGL(k_terrain_rays<true>, dim3(blocks_of(n_rays)), dim3(kBlock), 0, stream, terrain, r, n_rays, h);
    else
        hipLaunchKernelGGL(k_terrain_rays<false>, dim3(blocks_of(n_rays)), dim3(kBlock), 0, stream, terrain, r, n_rays, h);
    return hipGetLastError();
}

hipError_t launch_terrain_sweeps(const Terrain &terrain, const PolytopeTables &t, const void *sweeps, uint32_t n_sweeps, bool brute, const double *qrec,
                                 void *hits, hipStream_t stream)
{
    if (n_sweeps == 0)
        return hipSuccess;
    const xpbd_sweep *s = static_cast<const xpbd_sweep *>(sweeps);
    xpbd_sweep_hit *h = static_cast<xpbd_sweep_hit *>(hits);
    const dim3 blocks(blocks_of(n_sweeps, kBlock / kSweepLanes));
    if (brute)
        hipLaunchKernelGGL(k_terrain_sweeps<true>, blocks, dim3(kBlock), 0, stream, terrain, t, s, n_sweeps, qrec, h);
    else
        hipLaunchKernelGGL(k_terrain_sweeps<false>, blocks, dim3(kBlock), 0, stream, terrain, t, s, n_sweeps, qrec, h);
    return hipGetLastError();
}

hipError_t launch_terrain_overlap(const Terrain &terrain, const PolytopeTables &t, const void *queries, uint32_t n_queries, bool fill, const double *qrec,
                                  uint32_t *offsets, void *hits, uint32_t cap, hipStream_t stream)
{
    if (n_queries == 0)
        return hipSuccess;
    const xpbd_overlap_query *q = static_cast<const xpbd_overlap_query *>(queries);
    xpbd_overlap_hit *h = static_cast<xpbd_overlap_hit *>(hits);
    if (fill)
        hipLaunchKernelGGL(k_terrain_overlap<true>, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, terrain, t, q, n_queries, qrec, offsets, h, cap);
    else
        hipLaunchKernelGGL(k_terrain_overlap<false>, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, terrain, t, q, n_queries, qrec, offsets, h, cap);
    return hipGetLastError();
}

hipError_t launch_terrain_distance(const TerrainHeights &terrain, const PolytopeTables &t, const void *queries, uint32_t n_queries, bool brute, void *hits,
                                   hipStream_t stream)
{
    if (n_queries == 0)
        return hipSuccess;
    const xpbd_distance_query *q = static_cast<const xpbd_distance_query *>(queries);
    xpbd_distance_hit *h = static_cast<xpbd_distance_hit *>(hits);
    const dim3 blocks(blocks_of(n_queries, kBlock / kDistanceLanes));
    if (brute)
        hipLaunchKernelGGL((k_terrain_distance<true, kDistanceLanes>), blocks, dim3(kBlock), 0, stream, terrain, t, q, n_queries, h);
    else
        hipLaunchKernelGGL((k_terrain_distance<false, kDistanceLanes>), blocks, dim3(kBlock), 0, stream, terrain, t, q, n_queries, h);
    return hipGetLastError();
}

} // namespace xpbd
