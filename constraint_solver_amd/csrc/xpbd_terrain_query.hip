// xpbd_terrain_query.hip -- the heightfield terrain in the scene queries (EXTENSION) for gfx950: the passes that put the terrain's
// answer next to the bodies' answer of a ray cast, a sweep and an overlap query (XPBD_QUERY_TERRAIN).
//
// Semantics: include/xpbd.h, "Terrain in the scene queries".  The terrain is the union of the prisms under its triangles; a
// ray's answer is the minimum over all triangles under (t, triangle).  A triangle's t is a function of the ray and the triangle
// alone, and neighbouring prisms compute the t of their shared wall and diagonal from the same expression, so the walk below
// -- which only chooses which cells are looked at -- cannot change a bit of the answer.  Nothing here writes anything but the
// callers' result arrays: no atomics, no LDS, no scratch memory of its own.
#include <cmath>
#include <cstdint>

#include "xpbd_query.h"
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

XPBD_HD bool finite3(Vec3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

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

} // namespace xpbd
