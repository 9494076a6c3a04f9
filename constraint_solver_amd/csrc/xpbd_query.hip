// xpbd_query.hip -- scene queries (EXTENSION) for gfx950: batched ray casts, overlap queries, sweep queries and distance queries against
// the world's bodies.
//
// Semantics: include/xpbd.h, "Scene queries"; layout of the work: xpbd_query.h.  Determinism: the winner of a ray is the
// minimum of its candidates under one total order -- (t, index) -- and a candidate's t is a function of the ray and the body
// alone, so neither the order in which the atomics of the grid build leave a cell's bodies nor a body being tested in
// several cells changes any bit.  Atomics count integers only.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include <type_traits>

#include "xpbd_clip.hpp"
#include "xpbd_query.h"
#include "xpbd_query_shared.hpp"
#include "xpbd_contacts.h"
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

uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

uint32_t brute_chunks(uint32_t n, uint32_t n_rays)
{
    const uint32_t tiles = (n_rays + kBruteRays - 1) / kBruteRays;
    uint32_t chunks = (kBruteBlocks + tiles - 1) / (tiles ? tiles : 1);
    const uint32_t most = blocks_of(n) ? blocks_of(n) : 1; // at least one body block (kBlock bodies) per workgroup
    return chunks < 1 ? 1 : (chunks > most ? most : chunks);
}

uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v)
        p <<= 1;
    return p;
}

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

__device__ __forceinline__ Ray load_ray(const xpbd_ray *__restrict__ rays, uint32_t r)
{
    const xpbd_ray &x = rays[r];
    Ray ray;
    ray.o = Vec3{x.origin[0], x.origin[1], x.origin[2]};
    ray.d = Vec3{x.direction[0], x.direction[1], x.direction[2]};
    ray.tmax = x.max_distance;
    ray.ignore = x.ignore_body;
    const bool finite = isfinite(ray.o.x) && isfinite(ray.o.y) && isfinite(ray.o.z) && isfinite(ray.d.x) && isfinite(ray.d.y) &&
                        isfinite(ray.d.z);
    const bool moving = ray.d.x != 0.0 || ray.d.y != 0.0 || ray.d.z != 0.0;
    ray.valid = finite && moving && ray.tmax >= 0.0; // (a NaN max_distance fails the comparison; +inf passes)
    return ray;
}

__device__ __forceinline__ BodyQ load_body(const double *__restrict__ rec, uint32_t i)
{
    const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kQueryRecDoubles);
    const double2 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4], f = r[5];
    return BodyQ{Vec3{a.x, a.y, b.x}, Quat{b.y, c.x, c.y, d.x}, Vec3{d.y, e.x, e.y}, f.x};
}

// Conservative sphere test: false only if the ray certainly misses the body's bounding sphere.
__device__ __forceinline__ bool may_reach(const Ray &ray, const BodyQ &q)
{
    const Vec3 w = q.centre - ray.o;
    const double w2 = dot(w, w), wd = dot(w, ray.d), dd = dot(ray.d, ray.d);
    const double r2 = q.radius * q.radius * kSphereSlack;
    if (w2 <= r2)
        return true; // the origin is inside (or close to) the sphere
    if (wd < 0.0)
        return false; // outside the sphere and moving away from its centre
    const double line2 = w2 - wd * (wd / dd);
    return line2 <= r2 + 1e-12 * w2;
}

__device__ __forceinline__ void test_body(const Ray &ray, const double *__restrict__ rec, const uint32_t *__restrict__ shape_id,
                                          const uint32_t *__restrict__ gid, const PolytopeTables &t, uint32_t i, Best &best)
{
    const BodyQ q = load_body(rec, i);
    if (!(q.radius >= 0.0))
        return;
    const uint32_t id = gid ? gid[i] : i;
    if (id == ray.ignore || !may_reach(ray, q))
        return;
    double th;
    uint32_t face;
    if (ray_body(ray, q, t, shape_id[i], th, face) && better(th, id, best))
        best = Best{th, id, face, i, 0};
}

__device__ __forceinline__ void write_hit(const Ray &ray, const Best &best, const double *__restrict__ rec, const uint32_t *__restrict__ shape_id,
                                          const PolytopeTables &t, xpbd_ray_hit *__restrict__ hit)
{
    xpbd_ray_hit h;
    h.body = best.id;
    h.face = best.face;
    h.distance = best.t;
    h.point[0] = h.point[1] = h.point[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (best.id != XPBD_NO_HIT) {
        const Vec3 p = ray.o + ray.d * best.t;
        h.point[0] = p.x, h.point[1] = p.y, h.point[2] = p.z;
        if (best.face != XPBD_RAY_INSIDE) {
            const BodyQ q = load_body(rec, best.slot);
            const double *pl = t.planes + 4 * (size_t)(t.desc[shape_id[best.slot]].face0 + best.face);
            const Vec3 n = conjugate(q.inv_rot) * Vec3{pl[0], pl[1], pl[2]}; // f.rotation = conjugate(inv.rotation), exactly
            h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
        }
    } else {
        h.face = XPBD_NO_HIT;
        h.distance = INFINITY;
    }
    *hit = h;
}

// ---- grid build -------------------------------------------------------------------------------------------------------
// Inverse frame and bounding sphere of every body, and per workgroup the largest radius and the box of the spheres.
__global__ void __launch_bounds__(kBlock) k_query_bodies(BodyArrays b, PolytopeTables t, const uint32_t *__restrict__ gid,
                                                         RayFilter filter, double *__restrict__ rec, double *__restrict__ partials)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double v[7] = {0.0, DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX}; // rmax, min xyz, max xyz
    if (i < b.n) {
        const Frame f = body_frame(b, i);
        const Frame inv = inverse(f);
        const uint32_t sid = b.shape_id[i];
        const double *cc = t.centroids + 3 * (size_t)sid;
        const Vec3 c = f * Vec3{cc[0], cc[1], cc[2]};
        const double r = t.radii[sid];
        const bool finite = isfinite(f.position.x) && isfinite(f.position.y) && isfinite(f.position.z) && isfinite(f.rotation.s) &&
                            isfinite(f.rotation.x) && isfinite(f.rotation.y) && isfinite(f.rotation.z) && isfinite(c.x) &&
                            isfinite(c.y) && isfinite(c.z);
        const uint32_t group = filter.filter ? filter.filter[i].x : ~0u;
        const bool able = finite && (!gid || gid[i] != XPBD_NO_HIT) && (!filter.masked || (group & filter.mask) != 0);
        double2 *o = reinterpret_cast<double2 *>(rec + (size_t)i * kQueryRecDoubles);
        o[0] = double2{inv.position.x, inv.position.y};
        o[1] = double2{inv.position.z, inv.rotation.s};
        o[2] = double2{inv.rotation.x, inv.rotation.y};
        o[3] = double2{inv.rotation.z, c.x};
        o[4] = double2{c.y, c.z};
        o[5] = double2{able ? r : -1.0, 0.0};
        if (able) {
            v[0] = r;
            v[1] = c.x - r, v[2] = c.y - r, v[3] = c.z - r;
            v[4] = c.x + r, v[5] = c.y + r, v[6] = c.z + r;
        }
    }
    __shared__ double part[kBlock / 64][7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        double x = v[q];
        for (uint32_t off = 32; off; off >>= 1) {
            const double o = __shfl_xor(x, off, 64);
            x = (q >= 1 && q <= 3) ? (o < x ? o : x) : (o > x ? o : x);
        }
        if ((threadIdx.x & 63u) == 0)
            part[threadIdx.x >> 6][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const uint32_t q = threadIdx.x;
        double x = part[0][q];
        for (uint32_t w = 1; w < kBlock / 64; ++w) {
            const double o = part[w][q];
            x = (q >= 1 && q <= 3) ? (o < x ? o : x) : (o > x ? o : x);
        }
        partials[(size_t)blockIdx.x * 7 + q] = x;
    }
}

// One workgroup: the grid of this call from the partials.
__global__ void __launch_bounds__(kBlock) k_query_grid(const double *__restrict__ partials, uint32_t n_partials, uint32_t table_size,
                                                       QueryGrid *__restrict__ grid)
{
    __shared__ double part[kBlock / 64][7];
    double v[7] = {0.0, DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (uint32_t k = threadIdx.x; k < n_partials; k += kBlock)
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const double o = partials[(size_t)k * 7 + q];
            v[q] = (q >= 1 && q <= 3) ? (o < v[q] ? o : v[q]) : (o > v[q] ? o : v[q]);
        }
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        double x = v[q];
        for (uint32_t off = 32; off; off >>= 1) {
            const double o = __shfl_xor(x, off, 64);
            x = (q >= 1 && q <= 3) ? (o < x ? o : x) : (o > x ? o : x);
        }
        if ((threadIdx.x & 63u) == 0)
            part[threadIdx.x >> 6][q] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    double m[7];
    for (int q = 0; q < 7; ++q) {
        m[q] = part[0][q];
        for (uint32_t w = 1; w < kBlock / 64; ++w) {
            const double o = part[w][q];
            m[q] = (q >= 1 && q <= 3) ? (o < m[q] ? o : m[q]) : (o > m[q] ? o : m[q]);
        }
    }
    QueryGrid g{};
    g.mask = table_size - 1;
    const bool any = m[1] <= m[4]; // some body can be hit
    g.edge = 2.0 * m[0] * kEdgeScale;
    g.pad = m[0] * kPadScale;
    bool fits = any && m[0] > 0.0 && isfinite(g.edge);
    double cells = 1.0;
    for (int a = 0; a < 3 && fits; ++a) {
        const double lo = floor((m[1 + a] - g.pad) / g.edge), hi = floor((m[4 + a] + g.pad) / g.edge);
        if (!(lo >= -kMaxCell && hi <= kMaxCell && hi - lo < kMaxDim)) {
            fits = false;
            break;
        }
        g.lo[a] = (int32_t)lo;
        g.dims[a] = (uint32_t)(hi - lo) + 1u;
        cells *= (double)g.dims[a];
    }
    g.mode = !any ? kEmpty : (fits ? kGrid : kEveryBody);
    g.dense = cells <= (double)table_size ? 1u : 0u;
    *grid = g;
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

// Every body into every cell its padded sphere box overlaps: FILL = false counts the cells' populations, true lists the bodies.
template <bool FILL>
__global__ void __launch_bounds__(kBlock) k_query_bin(uint32_t n, const double *__restrict__ rec, const QueryGrid *__restrict__ grid,
                                                      uint32_t *__restrict__ cell_start, uint32_t *__restrict__ cell_fill,
                                                      uint32_t *__restrict__ items)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const QueryGrid g = *grid;
    if (g.mode != kGrid)
        return;
    const BodyQ q = load_body(rec, i);
    if (!(q.radius >= 0.0))
        return;
    const double c[3] = {q.centre.x, q.centre.y, q.centre.z};
    int32_t lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = clamp_axis(g, a, floor((c[a] - q.radius - g.pad) / g.edge));
        hi[a] = clamp_axis(g, a, floor((c[a] + q.radius + g.pad) / g.edge));
        hi[a] = hi[a] > lo[a] + 1 ? lo[a] + 1 : hi[a]; // (never binding, see kEdgeScale; `items` holds 8 entries per body)
    }
    for (int32_t z = lo[2]; z <= hi[2]; ++z)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
            for (int32_t x = lo[0]; x <= hi[0]; ++x) {
                const uint32_t key = query_key(g, x, y, z);
                if (FILL)
                    items[cell_start[key] + atomicAdd(&cell_fill[key], 1u)] = i;
                else
                    atomicAdd(&cell_start[key], 1u);
            }
}

// ---- traversal: one lane per ray ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_query_walk(const xpbd_ray *__restrict__ rays, uint32_t n_rays, uint32_t n,
                                                       const double *__restrict__ rec, const uint32_t *__restrict__ shape_id,
                                                       const uint32_t *__restrict__ gid, PolytopeTables t,
                                                       const QueryGrid *__restrict__ grid, const uint32_t *__restrict__ cell_start,
                                                       const uint32_t *__restrict__ items, xpbd_ray_hit *__restrict__ hits)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays)
        return;
    const Ray ray = load_ray(rays, r);
    const QueryGrid g = *grid;
    Best best = no_hit();
    if (ray.valid && g.mode == kEveryBody) {
        for (uint32_t i = 0; i < n; ++i)
            test_body(ray, rec, shape_id, gid, t, i, best);
    } else if (ray.valid && g.mode == kGrid) {
        const double o[3] = {ray.o.x, ray.o.y, ray.o.z}, d[3] = {ray.d.x, ray.d.y, ray.d.z};
        double t_near, t_far;
        if (clip_to_grid(g, o, d, ray.tmax, 0.0, t_near, t_far)) {
            int32_t cell[3], step[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // A zero component is its own case: the ray stays in the slab of cells of its origin, and when the origin
                // lies ON a cell face (o = k * edge exactly) that is cell k -- every body touching the face is listed
                // there too, because binned boxes are padded.
                const double p = d[a] == 0.0 ? o[a] : o[a] + t_near * d[a];
                cell[a] = clamp_axis(g, a, floor(p / g.edge));
                step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
            }
            double t_enter = t_near;
            for (;;) {
                if (t_enter > best.t) // strict: a tie in the next cell can still win on the smaller index
                    break;
                const uint32_t key = query_key(g, cell[0], cell[1], cell[2]);
                const uint32_t s1 = cell_start[key + 1];
                for (uint32_t s = cell_start[key]; s < s1; ++s)
                    test_body(ray, rec, shape_id, gid, t, items[s], best);
                double t_next;
                const int axis = next_face(g, cell, step, o, d, t_next);
                if (axis < 0 || t_next > t_far)
                    break;
                cell[axis] += step[axis];
                if (cell[axis] < g.lo[axis] || cell[axis] >= g.lo[axis] + (int32_t)g.dims[axis])
                    break;
                t_enter = t_next;
            }
        }
    }
    write_hit(ray, best, rec, shape_id, t, hits + r);
}

// ---- brute force: workgroup (tile of kBruteRays rays, chunk of bodies) --------------------------------------------------
__device__ __forceinline__ void wave_min(Best &b)
{
    for (uint32_t off = 32; off; off >>= 1) {
        Best o;
        o.t = __shfl_xor(b.t, off, 64);
        o.id = __shfl_xor(b.id, off, 64);
        o.face = __shfl_xor(b.face, off, 64);
        o.slot = __shfl_xor(b.slot, off, 64);
        o.pad = 0;
        if (better(o.t, o.id, b))
            b = o;
    }
}

__global__ void __launch_bounds__(kBlock) k_query_brute(const xpbd_ray *__restrict__ rays, uint32_t n_rays, uint32_t n, uint32_t chunk_len,
                                                        const double *__restrict__ rec, const uint32_t *__restrict__ shape_id,
                                                        const uint32_t *__restrict__ gid, PolytopeTables t, Best *__restrict__ partial)
{
    const uint32_t r0 = blockIdx.x * kBruteRays, chunk = blockIdx.y, chunks = gridDim.y;
    __shared__ Best wave_best[kBlock / 64][kBruteRays];
    Ray ray[kBruteRays];
    Best best[kBruteRays];
#pragma unroll
    for (uint32_t q = 0; q < kBruteRays; ++q) {
        ray[q] = r0 + q < n_rays ? load_ray(rays, r0 + q) : Ray{};
        if (r0 + q >= n_rays)
            ray[q].valid = false;
        best[q] = no_hit();
    }
    const uint32_t begin = chunk * chunk_len, end = begin + chunk_len < n ? begin + chunk_len : n;
    for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) {
#pragma unroll
        for (uint32_t q = 0; q < kBruteRays; ++q)
            if (ray[q].valid)
                test_body(ray[q], rec, shape_id, gid, t, i, best[q]);
    }
#pragma unroll
    for (uint32_t q = 0; q < kBruteRays; ++q) {
        wave_min(best[q]);
        if ((threadIdx.x & 63u) == 0)
            wave_best[threadIdx.x >> 6][q] = best[q];
    }
    __syncthreads();
    if (threadIdx.x < kBruteRays && r0 + threadIdx.x < n_rays) {
        const uint32_t q = threadIdx.x;
        Best b = wave_best[0][q];
        for (uint32_t w = 1; w < kBlock / 64; ++w)
            if (better(wave_best[w][q].t, wave_best[w][q].id, b))
                b = wave_best[w][q];
        partial[(size_t)(r0 + q) * chunks + chunk] = b;
    }
}

// One wave per ray: the partials of its workgroups (up to kBruteBlocks of them for a single ray) reduced across the lanes.
__global__ void __launch_bounds__(64) k_query_brute_finish(const xpbd_ray *__restrict__ rays, uint32_t chunks, const Best *__restrict__ partial,
                                                           const double *__restrict__ rec, const uint32_t *__restrict__ shape_id,
                                                           PolytopeTables t, xpbd_ray_hit *__restrict__ hits)
{
    const uint32_t r = blockIdx.x;
    Best best = no_hit();
    for (uint32_t c = threadIdx.x; c < chunks; c += 64) {
        const Best b = partial[(size_t)r * chunks + c];
        if (better(b.t, b.id, best))
            best = b;
    }
    wave_min(best);
    if (threadIdx.x == 0)
        write_hit(load_ray(rays, r), best, rec, shape_id, t, hits + r);
}

// ---- overlap queries: convex volumes against the bodies ------------------------------------------------------------------
// Semantics: include/xpbd.h, "Overlap queries".  One (query, body) pair is decided by three steps -- ignore_body and the group
// mask, the tight bounding spheres, the decision part of the SAT -- and both paths run the same routines for them, so the set
// of hits of a query does not depend on the path.  Neither does its order: the brute-force path visits the bodies in
// ascending index and reports them as it goes; the grid path reports them in cell order and k_overlap_sort brings every
// segment into ascending index (indices are distinct).  Every pass is run twice: once to count, once to fill, with an
// exclusive scan in between -- no list whose length the host would have to learn.
constexpr uint32_t kOverlapRecDoubles = 4; // per query: sphere centre xyz, radius (< 0: the query reports nothing)
constexpr uint32_t kNoBody = 0xFFFFFFFFu;
static_assert(sizeof(xpbd_overlap_query) == 72 && sizeof(xpbd_overlap_hit) == 16, "xpbd_overlap_query is 72 bytes, xpbd_overlap_hit 16");

// One lane per query: its bounding sphere, and whether it can report anything (finite frame, shape of the table).
__global__ void __launch_bounds__(kBlock) k_overlap_queries(const xpbd_overlap_query *__restrict__ queries, uint32_t n_queries, PolytopeTables t,
                                                            double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries)
        return;
    const xpbd_overlap_query &x = queries[q];
    const Frame f{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (x.shape < t.n_shapes) {
        const double *cc = t.centroids + 3 * (size_t)x.shape;
        c = f * Vec3{cc[0], cc[1], cc[2]};
        const bool finite = isfinite(f.position.x) && isfinite(f.position.y) && isfinite(f.position.z) && isfinite(f.rotation.s) &&
                            isfinite(f.rotation.x) && isfinite(f.rotation.y) && isfinite(f.rotation.z) && isfinite(c.x) && isfinite(c.y) &&
                            isfinite(c.z);
        const double rs = t.radii[x.shape];
        if (finite && rs >= 0.0)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

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

struct OverlapArgs : PassArgs {
    const xpbd_overlap_query *queries;
    uint32_t *offsets;          // count pass: offsets[q] = hits of q; fill pass: the scanned array
    xpbd_overlap_hit *hits;
    uint32_t cap;
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

// Count (FILL = false) or list (true) the hits of every query: one group of L lanes per query, 64 / L queries per wave.  The
// lanes of a group run steps 1 and 2 for one candidate each -- on the grid path each lane walks cells of its own out of the
// box of cells the query's sphere covers -- and the group then decides the survivors one after the other (step 3).
template <uint32_t L, uint32_t V, bool FILL>
__global__ void __launch_bounds__(64) k_overlap_pass(BodyArrays b, PolytopeTables t, OverlapArgs a)
{
    constexpr uint32_t PW = 64 / L;
    __shared__ OverlapLds<V> s_all[PW];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PW + group;
    if (q >= a.n)
        return;
    OverlapLds<V> &s = s_all[group];
    const double2 *qr = reinterpret_cast<const double2 *>(a.qrec + (size_t)q * kOverlapRecDoubles);
    const double2 q0 = qr[0], q1 = qr[1];
    const Vec3 cq{q0.x, q0.y, q1.x};
    const double rq = q1.y;
    // A segment the caller's buffer cuts short is listed in ascending order straight away (its first entries are what the
    // caller gets, and the sort needs whole segments); segments past the buffer are not listed at all.
    bool ordered = a.brute != 0;
    uint32_t base = 0, room = 0xFFFFFFFFu;
    if (FILL) {
        base = a.offsets[q];
        const uint32_t end = a.offsets[q + 1];
        if (end == base || base >= a.cap)
            return;
        ordered = ordered || end > a.cap;
        room = a.cap - base;
    }
    uint32_t count = 0;
    if (rq >= 0.0) {
        const xpbd_overlap_query &x = a.queries[q];
        const Frame fq{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
        const Frame fq_inv = inverse(fq);
        const uint32_t sq = x.shape, ignore = x.ignore_body, mask = x.mask;
        {
            const ShapeDesc dq = t.desc[sq];
            for (uint32_t vtx = lane; vtx < dq.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(dq.vert0 + vtx);
                st3(s.world[0], vtx, fq * Vec3{v[0], v[1], v[2]});
            }
        }
        // steps 1 and 2 of body i (one lane)
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            if (!admit_record(a, i, ignore, mask, centre, radius))
                return false;
            const Vec3 between = centre - cq;
            const double reach = rq + radius;
            return dot(between, between) < reach * reach;
        };
        // step 3 of the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                uint32_t feature = 0;
                double separation = 0.0;
                if (overlap_decide<L>(s, t, fq, fq_inv, sq, body_frame(b, i), b.shape_id[i], lane, feature, separation)) {
                    if (FILL && lane == 0 && count < room) {
                        xpbd_overlap_hit h;
                        h.body = a.gid ? a.gid[i] : i;
                        h.feature = feature;
                        h.separation = separation;
                        a.hits[base + count] = h;
                    }
                    ++count;
                }
            });
        };
        // the cells of the query on the grid, and whether walking them beats looking at every body
        QueryGrid g{};
        int32_t qlo[3] = {0, 0, 0};
        uint32_t qdim[3] = {1, 1, 1};
        bool walk = false;
        if (!ordered) {
            g = *a.grid;
            if (g.mode == kGrid) {
                const double c[3] = {cq.x, cq.y, cq.z};
                double cells = 1.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    qlo[ax] = clamp_axis(g, ax, floor((c[ax] - rq - g.pad) / g.edge));
                    const int32_t hi = clamp_axis(g, ax, floor((c[ax] + rq + g.pad) / g.edge));
                    qdim[ax] = (uint32_t)(hi - qlo[ax]) + 1u;
                    cells *= (double)qdim[ax];
                }
                walk = cells <= (double)g.mask + 1.0; // at most the cells a dense grid can have; beyond that, every body in turn
            }
        }
        if (walk)
            walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit, [](int, int32_t, int32_t) { return false; }, decide);
        else if (ordered || g.mode != kEmpty)
            // (its own loop, like the sweep pass's; see DESIGN, "One walk, measured")
            for (uint32_t i0 = 0; i0 < b.n && count < room; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
    }
    if (!FILL && lane == 0)
        a.offsets[q] = count;
}

// Every query's segment into ascending body order, one workgroup per query.  Indices are distinct: up to kOverlapSortStage
// entries are staged in LDS and each goes to the place its rank names; longer segments are sorted where they are, in global
// memory, by a bitonic network whose comparators all point upwards (entries past the end count as +inf and never move).
__global__ void __launch_bounds__(kBlock) k_overlap_sort(const uint32_t *__restrict__ offsets, xpbd_overlap_hit *__restrict__ hits, uint32_t cap)
{
    __shared__ xpbd_overlap_hit stage[kOverlapSortStage];
    const uint32_t b0 = offsets[blockIdx.x], b1 = offsets[blockIdx.x + 1];
    if (b1 > cap || b1 - b0 < 2)
        return; // (a segment the buffer cuts short was listed in order)
    const uint32_t len = b1 - b0;
    xpbd_overlap_hit *seg = hits + b0;
    if (len <= kOverlapSortStage) {
        for (uint32_t e = threadIdx.x; e < len; e += kBlock)
            stage[e] = seg[e];
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < len; e += kBlock) {
            const uint32_t id = stage[e].body;
            uint32_t rank = 0;
            for (uint32_t o = 0; o < len; ++o)
                rank += stage[o].body < id ? 1u : 0u;
            seg[rank] = stage[e];
        }
        return;
    }
    for (uint32_t k = 2; (k >> 1) < len; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < len; i += kBlock) {
                const uint32_t p = j == (k >> 1) ? i ^ (k - 1u) : i ^ j; // merge of two sorted runs: mirrored; then half-cleaners
                if (p > i && p < len) {
                    const xpbd_overlap_hit lo = seg[i], hi = seg[p];
                    if (lo.body > hi.body) {
                        seg[i] = hi;
                        seg[p] = lo;
                    }
                }
            }
            __syncthreads();
        }
}

// ---- sweep queries: a convex volume translated along a segment -------------------------------------------------------------
// Semantics: include/xpbd.h, "Sweep queries".  The volume A at fa + t * d against the resting body B is, over every axis the SAT
// walks, one linear constraint "separation = s + t * v": the ray's slab test (ray_body) over the faces of A, the faces of B and
// both signs of every edge-direction pair.  The winner of a sweep is the minimum of its candidates under (t, index), and a
// candidate's t is a function of the sweep and the body alone, so neither the path nor how often a body is tested changes a bit.
static_assert(sizeof(xpbd_sweep) == 104 && sizeof(xpbd_sweep_hit) == 72, "xpbd_sweep is 104 bytes, xpbd_sweep_hit 72");
constexpr double kSweepReach = 4.0;   // volumes wider than this many cell edges look at every body instead of walking cells
constexpr double kSweepMargin = 0.01; // the centre line is clipped to the grid's box grown by the radius and this part of a cell

struct Sweep {
    Frame f;
    Vec3 d;
    double tmax;
    uint32_t shape, ignore, mask;
};

__device__ __forceinline__ Sweep load_sweep(const xpbd_sweep *__restrict__ sweeps, uint32_t q)
{
    const xpbd_sweep &x = sweeps[q];
    return Sweep{Frame{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}},
                 Vec3{x.direction[0], x.direction[1], x.direction[2]}, x.max_distance, x.shape, x.ignore_body, x.mask};
}

// One lane per sweep: the bounding sphere of the volume at t = 0 (the layout of k_overlap_queries) and whether the sweep can hit
// anything -- a shape of the table, a finite frame and direction, a direction that moves, a max_distance >= 0 -- as radius >= 0.
__global__ void __launch_bounds__(kBlock) k_sweep_queries(const xpbd_sweep *__restrict__ sweeps, uint32_t n_sweeps, PolytopeTables t,
                                                          double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_sweeps)
        return;
    const Sweep sw = load_sweep(sweeps, q);
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (sw.shape < t.n_shapes) {
        const double *cc = t.centroids + 3 * (size_t)sw.shape;
        c = sw.f * Vec3{cc[0], cc[1], cc[2]};
        const bool finite = isfinite(sw.f.position.x) && isfinite(sw.f.position.y) && isfinite(sw.f.position.z) && isfinite(sw.f.rotation.s) &&
                            isfinite(sw.f.rotation.x) && isfinite(sw.f.rotation.y) && isfinite(sw.f.rotation.z) && isfinite(c.x) &&
                            isfinite(c.y) && isfinite(c.z) && isfinite(sw.d.x) && isfinite(sw.d.y) && isfinite(sw.d.z);
        const bool moving = sw.d.x != 0.0 || sw.d.y != 0.0 || sw.d.z != 0.0;
        const double rs = t.radii[sw.shape];
        if (finite && moving && sw.tmax >= 0.0 && rs >= 0.0) // (a NaN max_distance fails the comparison; +inf passes)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

// Conservative swept-sphere test: false only if the volume's bounding sphere, its centre moving from c along d over [0, t_end],
// certainly stays clear of the body's.  Never part of the definition: the slack (a relative 1e-6 on the reach, 1e-12 on the
// distance) is far above the rounding of the test and of the spheres, so no pair the routine below would hit is dropped.
__device__ __forceinline__ bool sweep_may_reach(Vec3 c, double rq, Vec3 d, double t_end, Vec3 cb, double rb)
{
    const Vec3 w = cb - c;
    const double reach = rq + rb;
    const double w2 = dot(w, w), wd = dot(w, d), dd = dot(d, d);
    const double bound = reach * reach * kSphereSlack + 1e-12 * w2;
    if (!(w2 > bound))
        return true; // in reach at the start
    if (wd < 0.0)
        return false; // out of reach and moving away
    const double ts = wd / dd;
    if (ts > t_end) { // the closest point of the segment is its end
        const Vec3 e = w - d * t_end;
        return !(dot(e, e) > bound);
    }
    return !(w2 - wd * ts > bound);
}

// The routine of one (sweep, body) pair by a group of L lanes.  A's world-space vertices are in s.world[0] already; t_cap is the
// sweep's max_distance or the best t so far, whichever is smaller (a pair that enters later cannot win, and an equal t still
// passes).  True on a hit, with its t and the position of the entering constraint in the order of the definition (kNoBody: the
// volume overlaps the body at the start).  Every lane of the group returns the same values.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool sweep_decide(Lds &s, const PolytopeTables &t, const Frame &fa, const Frame &fa_inv, uint32_t sa, Vec3 d, Vec3 d_a,
                                             const Frame &fb, uint32_t sb, uint32_t lane, double t_cap, double &t_hit, uint32_t &entering)
{
    constexpr uint32_t H = L / 2;
    const ShapeDesc da = t.desc[sa], db = t.desc[sb];
    if (da.n_verts == 0 || db.n_verts == 0 || da.n_faces == 0 || db.n_faces == 0)
        return false;
    const Frame fb_inv = inverse(fb);
    const Vec3 d_b = fb_inv.rotation * d;
    const uint32_t half = lane / H, k = lane % H; // first half of the group works for A, second for B
    stage_pair(s, t, da, db, fa_inv, fb, fb_inv, half, k, H);

    double t_lo = -INFINITY, t_hi = t_cap;
    uint32_t enter = kNoBody;
    bool miss = false;
    // one constraint, position `at` in the order of the definition (ascending on every lane: the first maximum stays)
    auto constrain = [&](double sep, double vel, uint32_t at) {
        if (sep != sep || vel != vel) {
            miss = true;
        } else if (vel < 0.0) {
            const double tk = (-sep) / vel;
            if (tk > t_lo) {
                t_lo = tk;
                enter = at;
            }
        } else if (vel > 0.0) {
            const double tk = (-sep) / vel;
            t_hi = tk < t_hi ? tk : t_hi;
        } else if (sep >= 0.0) {
            miss = true;
        }
    };
    // the group's t_lo (first maximum), t_hi and verdict so far; true: a miss for good
    auto settle = [&]() -> bool {
        reduce_max_first(t_lo, enter, L);
        for (uint32_t off = L >> 1; off; off >>= 1) {
            const double o = partner(t_hi, off);
            t_hi = o < t_hi ? o : t_hi;
        }
        return group_bits<L>(__ballot(miss)) != 0 || t_lo > t_hi;
    };

    // ---- faces: A's on the first half (against B's vertices in A's space), B's on the second ------------------------------
    {
        const ShapeDesc dm = half ? db : da;
        const uint32_t n_other = half ? da.n_verts : db.n_verts;
        const Vec3 d_m = half ? d_b : d_a;
        for (uint32_t f = k; f < dm.n_faces; f += H) {
            const double *pl = t.planes + 4 * (size_t)(dm.face0 + f);
            const Vec3 n{pl[0], pl[1], pl[2]};
            double low = dot(n, ld3(s.local[half ^ 1u], 0));
            for (uint32_t v = 1; v < n_other; ++v) {
                const double x = dot(n, ld3(s.local[half ^ 1u], v));
                low = x < low ? x : low;
            }
            const double w = dot(n, d_m);
            constrain(low - pl[3], half ? w : -w, half ? da.n_faces + f : f);
        }
    }
    if (settle())
        return false;

    // ---- edge axes: (unique edge direction of A) x (unique edge direction of B), both signs -------------------------------
    const bool dirs_staged = stage_edge_dirs<L>(s, t, da, db, fa, fb, lane);
    const uint32_t total = da.n_dirs * db.n_dirs, edge0 = da.n_faces + db.n_faces;
    for (uint32_t q = lane; q < total; q += L) {
        const uint32_t i = q / db.n_dirs, j = q - i * db.n_dirs;
        const Vec3 n = edge_axis(s, dirs_staged, t, da, db, fa, fb, i, j);
        if (!(fabs(n.x) <= DBL_MAX && fabs(n.y) <= DBL_MAX && fabs(n.z) <= DBL_MAX))
            continue; // parallel directions: no axis
        double hi_a = dot(ld3(s.world[0], 0), n), lo_a = hi_a, hi_b = dot(ld3(s.world[1], 0), n), lo_b = hi_b;
        for (uint32_t v = 1; v < da.n_verts; ++v) {
            const double x = dot(ld3(s.world[0], v), n);
            hi_a = x > hi_a ? x : hi_a;
            lo_a = x < lo_a ? x : lo_a;
        }
        for (uint32_t v = 1; v < db.n_verts; ++v) {
            const double x = dot(ld3(s.world[1], v), n);
            hi_b = x > hi_b ? x : hi_b;
            lo_b = x < lo_b ? x : lo_b;
        }
        const double w = dot(n, d);
        constrain(lo_b - hi_a, -w, edge0 + 2u * q);
        constrain(lo_a - hi_b, w, edge0 + 2u * q + 1u);
    }
    if (settle())
        return false;
    const bool initial = t_lo < 0.0;
    t_hit = initial ? 0.0 : t_lo;
    entering = initial ? kNoBody : enter;
    return t_hit <= t_hi;
}

struct SweepArgs : PassArgs {
    const xpbd_sweep *sweeps;
    xpbd_sweep_hit *hits;
};

// The closest body of every sweep: one group of L lanes per sweep, 64 / L sweeps per wave.  The lanes of a group admit one
// candidate each (ignore_body, the mask, the swept spheres) and the group then decides the survivors one after the other.  On
// the grid path the centre line is walked cell by cell as k_query_walk walks a ray, and for the time the centre spends in one
// cell the lanes share out the box of cells the volume's sphere covers meanwhile.
template <uint32_t L, uint32_t V>
__global__ void __launch_bounds__(64) k_sweep_pass(BodyArrays b, PolytopeTables t, SweepArgs a)
{
    constexpr uint32_t PW = 64 / L;
    __shared__ OverlapLds<V> s_all[PW];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PW + group;
    if (q >= a.n)
        return;
    OverlapLds<V> &s = s_all[group];
    const double2 *qr = reinterpret_cast<const double2 *>(a.qrec + (size_t)q * kOverlapRecDoubles);
    const double2 q0 = qr[0], q1 = qr[1];
    const Vec3 cq{q0.x, q0.y, q1.x};
    const double rq = q1.y;
    const Sweep sw = load_sweep(a.sweeps, q);
    Best best = no_hit(); // (face: the position of the entering constraint)
    Frame fq_inv{};
    Vec3 d_q{0.0, 0.0, 0.0};
    if (rq >= 0.0) {
        fq_inv = inverse(sw.f);
        d_q = fq_inv.rotation * sw.d;
        {
            const ShapeDesc dq = t.desc[sw.shape];
            for (uint32_t vtx = lane; vtx < dq.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(dq.vert0 + vtx);
                st3(s.world[0], vtx, sw.f * Vec3{v[0], v[1], v[2]});
            }
        }
        // may body i win? (one lane)
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            return admit_record(a, i, sw.ignore, sw.mask, centre, radius) &&
                   sweep_may_reach(cq, rq, sw.d, best.t < sw.tmax ? best.t : sw.tmax, centre, radius);
        };
        // the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                double th = 0.0;
                uint32_t entering = kNoBody;
                if (sweep_decide<L>(s, t, sw.f, fq_inv, sw.shape, sw.d, d_q, body_frame(b, i), b.shape_id[i], lane,
                                    best.t < sw.tmax ? best.t : sw.tmax, th, entering)) {
                    const uint32_t id = a.gid ? a.gid[i] : i;
                    if (better(th, id, best))
                        best = Best{th, id, entering, i, 0};
                }
            });
        };
        QueryGrid g{};
        if (!a.brute)
            g = *a.grid;
        if (a.brute || g.mode == kEveryBody || (g.mode == kGrid && !(rq <= kSweepReach * g.edge))) {
            for (uint32_t i0 = 0; i0 < b.n; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
        } else if (g.mode == kGrid) {
            const double o[3] = {cq.x, cq.y, cq.z}, d[3] = {sw.d.x, sw.d.y, sw.d.z};
            // clip the centre line to the grid's box grown by the volume's radius: [t_near, t_far].  Outside it the volume
            // reaches no body's sphere; the cells of the walk may lie outside the grid, the boxes below are clamped to it.
            double t_near, t_far;
            if (clip_to_grid(g, o, d, sw.tmax, rq + kSweepMargin * g.edge, t_near, t_far)) {
                int32_t cell[3], step[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double p = d[ax] == 0.0 ? o[ax] : o[ax] + t_near * d[ax];
                    // (within kSweepReach + 1 cells of the grid, by the clip; the bound keeps the conversion defined regardless)
                    double c = floor(p / g.edge);
                    const double c_lo = (double)g.lo[ax] - (kSweepReach + 2.0), c_hi = (double)g.lo[ax] + (double)g.dims[ax] + (kSweepReach + 2.0);
                    c = c < c_lo ? c_lo : (c > c_hi ? c_hi : c);
                    cell[ax] = (int32_t)c;
                    step[ax] = d[ax] > 0.0 ? 1 : (d[ax] < 0.0 ? -1 : 0);
                }
                double t_enter = t_near;
                // the previous stretch's box; none yet: empty whatever the sign of the grid's cell coordinates
                int32_t plo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, phi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
                for (;;) {
                    if (t_enter > best.t) // strict: a tie later on can still win on the smaller index
                        break;
                    // when the centre leaves this cell
                    double t_next;
                    const int axis = next_face(g, cell, step, o, d, t_next);
                    const double t_leave = t_next < t_far ? t_next : t_far;
                    // the box of cells the sphere covers while its centre runs over [t_enter, t_leave]
                    int32_t qlo[3];
                    uint32_t qdim[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double p0 = d[ax] == 0.0 ? o[ax] : o[ax] + t_enter * d[ax], p1 = d[ax] == 0.0 ? o[ax] : o[ax] + t_leave * d[ax];
                        const double c_min = p0 < p1 ? p0 : p1, c_max = p0 < p1 ? p1 : p0;
                        qlo[ax] = clamp_axis(g, ax, floor((c_min - rq - g.pad) / g.edge));
                        const int32_t hi = clamp_axis(g, ax, floor((c_max + rq + g.pad) / g.edge));
                        qdim[ax] = (uint32_t)(hi - qlo[ax]) + 1u;
                    }
                    // A body counts in one cell of this box (walk_cell_box), and not at all if the previous stretch's box held
                    // one of its cells -- the boxes that meet a body's cells are consecutive stretches (the centre moves one
                    // way on every axis), so it was looked at then, with a t_cap no smaller than now.  A test too many would
                    // change nothing.
                    walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit,
                                     [&](int ax, int32_t lo, int32_t hi) { return lo <= phi[ax] && hi >= plo[ax]; }, decide);
                    if (axis < 0 || t_next > t_far)
                        break;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        plo[ax] = qlo[ax];
                        phi[ax] = qlo[ax] + (int32_t)qdim[ax] - 1;
                    }
                    cell[axis] += step[axis];
                    t_enter = t_next;
                }
            }
        }
    }
    if (lane != 0)
        return;
    xpbd_sweep_hit h;
    h.body = best.id;
    h.feature = 0;
    h.face = XPBD_NO_HIT;
    h.reserved = 0;
    h.distance = INFINITY;
    h.position[0] = h.position[1] = h.position[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (best.id != XPBD_NO_HIT) {
        h.distance = best.t;
        const Vec3 p = sw.f.position + sw.d * best.t;
        h.position[0] = p.x, h.position[1] = p.y, h.position[2] = p.z;
        const uint32_t sb = b.shape_id[best.slot];
        const ShapeDesc da = t.desc[sw.shape], db = t.desc[sb];
        const uint32_t at = best.face;
        if (at == kNoBody) {
            h.feature = XPBD_SWEEP_INITIAL;
        } else {
            const Frame fb = body_frame(b, best.slot);
            Vec3 n;
            if (at < da.n_faces) {
                const double *pl = t.planes + 4 * (size_t)(da.face0 + at);
                h.feature = XPBD_FEATURE_FACE_A;
                h.face = at;
                n = -(sw.f.rotation * Vec3{pl[0], pl[1], pl[2]});
            } else if (at < da.n_faces + db.n_faces) {
                const double *pl = t.planes + 4 * (size_t)(db.face0 + (at - da.n_faces));
                h.feature = XPBD_FEATURE_FACE_B;
                h.face = at - da.n_faces;
                n = fb.rotation * Vec3{pl[0], pl[1], pl[2]};
            } else {
                const uint32_t e = at - da.n_faces - db.n_faces, pair = e >> 1, i = pair / db.n_dirs, j = pair - i * db.n_dirs;
                n = edge_axis_of_table(t, da, db, sw.f, fb, i, j);
                h.feature = XPBD_FEATURE_EDGES;
                n = (e & 1u) ? n : -n;
            }
            h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
        }
    }
    a.hits[q] = h;
}

// ---- distance queries: the body nearest to a convex volume or a point -------------------------------------------------------
// Semantics: include/xpbd.h, "Distance queries".  One (volume, body) pair is the overlap query's decision first and then the
// minimum of d2 over a fixed list of candidates -- vertex over face both ways, then every pair of edges -- under (d2, position in
// the list).  A pair's distance is a function of the query and the body alone and the winner of a query is the minimum under
// (distance, index), so neither the path nor how often a body is looked at changes a bit.
static_assert(sizeof(xpbd_distance_query) == 80 && sizeof(xpbd_distance_hit) == 96, "xpbd_distance_query is 80 bytes, xpbd_distance_hit 96");
constexpr uint32_t kOverlapAt = 0xFFFFFFFEu; // Best::face of a pair that is not separated (kNoBody: no candidate)

struct DistanceQ {
    Frame f;
    double dmax;
    uint32_t shape, ignore, mask;
};

__device__ __forceinline__ DistanceQ load_distance(const xpbd_distance_query *__restrict__ queries, uint32_t q)
{
    const xpbd_distance_query &x = queries[q];
    return DistanceQ{Frame{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}},
                     x.max_distance, x.shape, x.ignore_body, x.mask};
}

// The volume's shape as the candidate lists see it: the point volume is one vertex, no faces and one edge from it to itself.
__device__ __forceinline__ ShapeDesc volume_desc(const PolytopeTables &t, uint32_t shape)
{
    return shape == XPBD_DISTANCE_POINT ? ShapeDesc{0, 1, 0, 0, 0, 1, 0, 0} : t.desc[shape];
}

// One lane per query: the bounding sphere of the volume (the layout of k_overlap_queries; the point volume: its position, radius
// 0) and whether the query can find anything -- a shape of the table or the point, a finite frame, a max_distance >= 0 -- as
// radius >= 0.
__global__ void __launch_bounds__(kBlock) k_distance_queries(const xpbd_distance_query *__restrict__ queries, uint32_t n_queries, PolytopeTables t,
                                                             double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries)
        return;
    const DistanceQ dq = load_distance(queries, q);
    const bool point = dq.shape == XPBD_DISTANCE_POINT;
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (point || dq.shape < t.n_shapes) {
        c = dq.f.position;
        double rs = 0.0;
        if (!point) {
            const double *cc = t.centroids + 3 * (size_t)dq.shape;
            c = dq.f * Vec3{cc[0], cc[1], cc[2]};
            rs = t.radii[dq.shape];
        }
        const bool finite = isfinite(dq.f.position.x) && isfinite(dq.f.position.y) && isfinite(dq.f.position.z) && isfinite(dq.f.rotation.s) &&
                            isfinite(dq.f.rotation.x) && isfinite(dq.f.rotation.y) && isfinite(dq.f.rotation.z) && isfinite(c.x) &&
                            isfinite(c.y) && isfinite(c.z);
        if (finite && dq.dmax >= 0.0 && rs >= 0.0) // (a NaN max_distance fails the comparison; +inf passes)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

// The tight spheres of the overlap query's rule 2, with the body's sphere from its record.
__device__ __forceinline__ bool spheres_overlap(const double *__restrict__ rec, uint32_t i, Vec3 cq, double rq)
{
    const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kQueryRecDoubles);
    const double2 d = r[3], e = r[4], f = r[5];
    const Vec3 between = Vec3{d.y, e.x, e.y} - cq;
    const double reach = rq + f.x;
    return dot(between, between) < reach * reach;
}

// The routine of one (volume, body) pair by a group of L lanes.  A's world-space vertices are in s.world[0] already.  True if
// the pair has an answer at all: its distance and `at`, the position of the winning candidate in the order of the definition
// (kOverlapAt: not separated).  Every lane of the group returns the same values.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool distance_decide(Lds &s, const PolytopeTables &t, const Frame &fa, const Frame &fa_inv, uint32_t sa, const Frame &fb,
                                                uint32_t sb, bool spheres, uint32_t lane, double &dist, uint32_t &at)
{
    constexpr uint32_t H = L / 2;
    const bool point = sa == XPBD_DISTANCE_POINT;
    const ShapeDesc da = volume_desc(t, sa), db = t.desc[sb];
    if (da.n_verts == 0 || db.n_verts == 0)
        return false;
    // ---- 1. the overlap query's decision --------------------------------------------------------------------------------
    if (spheres && !point) {
        uint32_t feature = 0;
        double separation = 0.0;
        if (overlap_decide<L>(s, t, fa, fa_inv, sa, fb, sb, lane, feature, separation)) {
            dist = 0.0;
            at = kOverlapAt;
            return true;
        }
    }
    // (again after a SAT that got as far as its edge axes: those may stand where the vertices stood)
    const Frame fb_inv = inverse(fb);
    stage_pair(s, t, da, db, fa_inv, fb, fb_inv, lane / H, lane % H, H);
    if (spheres && point && db.n_faces) {
        const Vec3 p = ld3(s.local[0], 0);
        const double *pl = t.planes + 4 * (size_t)db.face0;
        double deepest = dot(Vec3{pl[0], pl[1], pl[2]}, p) - pl[3];
        for (uint32_t f = 1; f < db.n_faces; ++f) {
            pl += 4;
            const double x = dot(Vec3{pl[0], pl[1], pl[2]}, p) - pl[3];
            deepest = x > deepest ? x : deepest;
        }
        if (deepest < 0.0) {
            dist = 0.0;
            at = kOverlapAt;
            return true;
        }
    }
    // ---- 2 (a), (b): vertex over face, A's vertices over B's faces and then B's over A's, spread over the lanes ---------------
    double d2 = INFINITY;
    at = kNoBody;
    const uint32_t over_b = da.n_verts * db.n_faces, faces = over_b + db.n_verts * da.n_faces;
    for (uint32_t c = lane; c < faces; c += L) {
        const bool on_b = c < over_b;
        const uint32_t cc = on_b ? c : c - over_b, nf = on_b ? db.n_faces : da.n_faces;
        const uint32_t v = cc / nf, f = cc - v * nf;
        double h;
        Vec3 foot;
        if (vertex_over_face(t, on_b ? db.vert0 : da.vert0, (on_b ? db.face0 : da.face0) + f, ld3(s.local[on_b ? 0 : 1], v), d2, h, foot)) {
            d2 = h * h; // ascending c on this lane: the first minimum stays
            at = c;
        }
    }
    reduce_min_first(d2, at, L);
    // ---- 2 (c): every edge of A against every edge of B, spread over the lanes, from the faces' winner on -----------------
    const uint32_t pairs = da.n_edges * db.n_edges;
    for (uint32_t q = lane; q < pairs; q += L) {
        const uint32_t i = q / db.n_edges, j = q - i * db.n_edges;
        const uint32_t *eb = t.edges + 2 * (size_t)(db.edge0 + j);
        uint32_t a0 = 0, a1 = 0;
        if (!point) {
            const uint32_t *ea = t.edges + 2 * (size_t)(da.edge0 + i);
            a0 = ea[0], a1 = ea[1];
        }
        Vec3 ca, cb;
        const double x = segment_closest(ld3(s.world[0], a0), ld3(s.world[0], a1), ld3(s.world[1], eb[0]), ld3(s.world[1], eb[1]), ca, cb);
        if (x < d2) {
            d2 = x;
            at = faces + q;
        }
    }
    reduce_min_first(d2, at, L);
    if (at == kNoBody)
        return false;
    dist = sqrt(d2);
    return true;
}

struct DistanceArgs : PassArgs {
    const xpbd_distance_query *queries;
    xpbd_distance_hit *hits;
};

// The nearest body of every query: one group of L lanes per query, 64 / L queries per wave.  The lanes of a group admit one
// candidate each (ignore_body, the mask, the gap between the bounding spheres against min(max_distance, best so far)) and the
// group then decides the survivors one after the other.  On the grid path the lanes share out the cells the volume's sphere
// covers, then those the sphere grown by min(max_distance, best so far) covers beyond them.
template <uint32_t L, uint32_t V>
__global__ void __launch_bounds__(64) k_distance_pass(BodyArrays b, PolytopeTables t, DistanceArgs a)
{
    constexpr uint32_t PW = 64 / L;
    __shared__ OverlapLds<V> s_all[PW];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PW + group;
    if (q >= a.n)
        return;
    OverlapLds<V> &s = s_all[group];
    const double2 *qr = reinterpret_cast<const double2 *>(a.qrec + (size_t)q * kOverlapRecDoubles);
    const double2 q0 = qr[0], q1 = qr[1];
    const Vec3 cq{q0.x, q0.y, q1.x};
    const double rq = q1.y;
    const DistanceQ dq = load_distance(a.queries, q);
    const bool point = dq.shape == XPBD_DISTANCE_POINT;
    Best best = no_hit(); // (face: the position of the winning candidate)
    Frame fq_inv{};
    if (rq >= 0.0) {
        fq_inv = inverse(dq.f);
        if (point) {
            if (lane == 0)
                st3(s.world[0], 0, dq.f.position);
        } else {
            const ShapeDesc ds = t.desc[dq.shape];
            for (uint32_t vtx = lane; vtx < ds.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(ds.vert0 + vtx);
                st3(s.world[0], vtx, dq.f * Vec3{v[0], v[1], v[2]});
            }
        }
        // may body i win? (one lane)  Conservative: the gap between the spheres is a lower bound of the distance, and the sweep
        // pre-test's slack is far above the rounding of the test and of the spheres.  Never part of the definition.
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            if (!admit_record(a, i, dq.ignore, dq.mask, centre, radius))
                return false;
            const Vec3 w = centre - cq;
            const double w2 = dot(w, w), reach = rq + radius + (best.t < dq.dmax ? best.t : dq.dmax);
            return !(w2 > reach * reach * kSphereSlack + 1e-12 * w2);
        };
        // the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                double dist = 0.0;
                uint32_t at = kNoBody;
                if (distance_decide<L>(s, t, dq.f, fq_inv, dq.shape, body_frame(b, i), b.shape_id[i], spheres_overlap(a.rec, i, cq, rq), lane, dist,
                                       at) &&
                    dist <= dq.dmax) {
                    const uint32_t id = a.gid ? a.gid[i] : i;
                    if (better(dist, id, best))
                        best = Best{dist, id, at, i, 0};
                }
            });
        };
        QueryGrid g{};
        if (!a.brute)
            g = *a.grid;
        if (a.brute || g.mode == kEveryBody || (g.mode == kGrid && !(rq + dq.dmax <= kSweepReach * g.edge))) {
            for (uint32_t i0 = 0; i0 < b.n; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
        } else if (g.mode == kGrid) {
            const double c[3] = {cq.x, cq.y, cq.z};
            // the box of cells a sphere of radius `reach` about the volume's centre covers (at most 2 kSweepReach + 2 cells a side:
            // fewer than the smallest table has keys)
            auto cells_of = [&](double reach, int32_t(&lo)[3], uint32_t(&dim)[3]) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    lo[ax] = clamp_axis(g, ax, floor((c[ax] - reach - g.pad) / g.edge));
                    const int32_t hi = clamp_axis(g, ax, floor((c[ax] + reach + g.pad) / g.edge));
                    dim[ax] = (uint32_t)(hi - lo[ax]) + 1u;
                }
            };
            int32_t plo[3], qlo[3];
            uint32_t pdim[3], qdim[3];
            cells_of(rq, plo, pdim);
            walk_cell_box<L>(g, plo, pdim, a.cell_start, a.items, lane, admit, [](int, int32_t, int32_t) { return false; }, decide);
            // A body whose cells met the first box was looked at there, with a bound no smaller than now: not again.
            cells_of(rq + (best.t < dq.dmax ? best.t : dq.dmax), qlo, qdim);
            if (qdim[0] != pdim[0] || qdim[1] != pdim[1] || qdim[2] != pdim[2])
                walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit,
                                 [&](int ax, int32_t lo, int32_t hi) { return lo <= plo[ax] + (int32_t)pdim[ax] - 1 && hi >= plo[ax]; }, decide);
        }
    }
    if (lane != 0)
        return;
    xpbd_distance_hit h;
    h.body = best.id;
    h.feature = 0;
    h.index_a = h.index_b = XPBD_NO_HIT;
    h.distance = INFINITY;
    h.point_a[0] = h.point_a[1] = h.point_a[2] = 0.0;
    h.point_b[0] = h.point_b[1] = h.point_b[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (best.id != XPBD_NO_HIT) {
        h.distance = best.t;
        if (best.face == kOverlapAt) {
            h.feature = XPBD_DISTANCE_OVERLAP;
        } else {
            // the winning candidate once more, by the expressions that staged and measured it
            const uint32_t sb = b.shape_id[best.slot];
            const ShapeDesc da = volume_desc(t, dq.shape), db = t.desc[sb];
            const Frame fb = body_frame(b, best.slot), fb_inv = inverse(fb);
            auto world_a = [&](uint32_t v) {
                if (point)
                    return dq.f.position;
                const double *x = t.verts + 3 * (size_t)(da.vert0 + v);
                return dq.f * Vec3{x[0], x[1], x[2]};
            };
            auto world_b = [&](uint32_t v) {
                const double *x = t.verts + 3 * (size_t)(db.vert0 + v);
                return fb * Vec3{x[0], x[1], x[2]};
            };
            const uint32_t over_b = da.n_verts * db.n_faces, faces = over_b + db.n_verts * da.n_faces, at = best.face;
            Vec3 pa{0.0, 0.0, 0.0}, pb{0.0, 0.0, 0.0}, foot{0.0, 0.0, 0.0};
            double hh = 0.0;
            if (at < over_b) {
                const uint32_t v = at / db.n_faces, f = at - v * db.n_faces;
                pa = world_a(v);
                vertex_over_face(t, db.vert0, db.face0 + f, fb_inv * pa, INFINITY, hh, foot);
                pb = fb * foot;
                h.feature = XPBD_FEATURE_FACE_B, h.index_a = v, h.index_b = f;
            } else if (at < faces) {
                const uint32_t v = (at - over_b) / da.n_faces, f = (at - over_b) - v * da.n_faces;
                pb = world_b(v);
                vertex_over_face(t, da.vert0, da.face0 + f, fq_inv * pb, INFINITY, hh, foot);
                pa = dq.f * foot;
                h.feature = XPBD_FEATURE_FACE_A, h.index_a = f, h.index_b = v;
            } else {
                const uint32_t e = at - faces, i = e / db.n_edges, j = e - i * db.n_edges;
                const uint32_t *eb = t.edges + 2 * (size_t)(db.edge0 + j);
                uint32_t a0 = 0, a1 = 0;
                if (!point) {
                    const uint32_t *ea = t.edges + 2 * (size_t)(da.edge0 + i);
                    a0 = ea[0], a1 = ea[1];
                }
                segment_closest(world_a(a0), world_a(a1), world_b(eb[0]), world_b(eb[1]), pa, pb);
                h.feature = XPBD_FEATURE_EDGES, h.index_a = i, h.index_b = j;
            }
            h.point_a[0] = pa.x, h.point_a[1] = pa.y, h.point_a[2] = pa.z;
            h.point_b[0] = pb.x, h.point_b[1] = pb.y, h.point_b[2] = pb.z;
            if (best.t != 0.0) {
                const Vec3 n = (pa - pb) * (1.0 / best.t);
                h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
            }
        }
    }
    a.hits[q] = h;
}

} // namespace

QuerySizes query_scratch_bytes(uint32_t n, uint32_t n_rays, bool brute)
{
    QuerySizes q{};
    q.rec = (size_t)(n ? n : 1) * kQueryRecDoubles * 8;
    q.partials = (size_t)(blocks_of(n) + 1) * 7 * 8;
    q.grid = sizeof(QueryGrid);
    q.table_size = next_pow2(4 * (n > 256 ? n : 256));
    if (brute) {
        q.cell_start = q.cell_fill = q.items = q.scan_scratch = 8;
        const uint32_t tiles = (n_rays + kBruteRays - 1) / kBruteRays;
        q.brute = (size_t)(tiles ? tiles : 1) * kBruteRays * brute_chunks(n, n_rays) * sizeof(Best);
    } else {
        q.cell_start = (size_t)(q.table_size + 1) * 4;
        q.cell_fill = (size_t)q.table_size * 4;
        q.items = (size_t)8 * (n ? n : 1) * 4;
        q.scan_scratch = ((size_t)q.table_size / 1024 + 8) * 4;
        q.brute = 8;
    }
    return q;
}

hipError_t SceneQueryScratch::reserve(const QuerySizes &q, size_t in_bytes, size_t out_bytes, size_t offsets_bytes, hipStream_t stream) noexcept
{
    return reserve_after_sync(stream, {{rec, q.rec}, {partials, q.partials}, {grid, q.grid}, {cell_start, q.cell_start}, {cell_fill, q.cell_fill},
                                       {items, q.items}, {scan, q.scan_scratch}, {brute, q.brute}, {qrec, q.qrec}, {in, in_bytes},
                                       {out, out_bytes}, {offsets, offsets_bytes}});
}

QueryScratch SceneQueryScratch::view(uint32_t table_size) const
{
    return QueryScratch{rec.as<double>(),    partials.as<double>(), grid.ptr,  cell_start.as<uint32_t>(), cell_fill.as<uint32_t>(),
                        items.as<uint32_t>(), scan.as<uint32_t>(),   brute.ptr, qrec.as<double>(),         table_size};
}

namespace {
// The first pass of every call: the bodies' records and the partial bounds of their spheres.
void launch_query_bodies(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const RayFilter &filter, const QueryScratch &s,
                         hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_query_bodies, dim3(blocks_of(b.n)), dim3(kBlock), 0, stream, b, t, global_id, filter, s.rec, s.partials);
}

// The grid over the bodies' spheres: its dimensions, the cells' populations, their scan, the bodies grouped by cell.
hipError_t launch_query_grid(const BodyArrays &b, const QueryScratch &s, hipStream_t stream)
{
    QueryGrid *grid = static_cast<QueryGrid *>(s.grid);
    hipError_t e = hipMemsetAsync(s.cell_start, 0, (size_t)(s.table_size + 1) * 4, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(s.cell_fill, 0, (size_t)s.table_size * 4, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_query_grid, dim3(1), dim3(kBlock), 0, stream, s.partials, blocks_of(b.n), s.table_size, grid);
    hipLaunchKernelGGL(k_query_bin<false>, dim3(blocks_of(b.n)), dim3(kBlock), 0, stream, b.n, s.rec, grid, s.cell_start, s.cell_fill,
                       s.items);
    if ((e = launch_exclusive_scan(s.cell_start, s.table_size, s.scan_scratch, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_query_bin<true>, dim3(blocks_of(b.n)), dim3(kBlock), 0, stream, b.n, s.rec, grid, s.cell_start, s.cell_fill,
                       s.items);
    return hipSuccess;
}
PassArgs pass_args(const QueryScratch &s, const uint32_t *global_id, const uint2 *filter, uint32_t n, bool masked, bool brute)
{
    return PassArgs{s.qrec, s.rec, global_id, filter, static_cast<QueryGrid *>(s.grid), s.cell_start, s.items, n, masked ? 1u : 0u, brute ? 1u : 0u};
}

// Lanes per query (L) and vertex capacity (V) of the group kernels by the largest shape, as the SAT launchers of the contact
// pipeline choose theirs: launch(L, V, workgroups) with L and V as std::integral_constant, 64 / L queries per workgroup.
template <class Launch>
void with_group_shape(const PolytopeTables &t, uint32_t n_queries, Launch &&launch)
{
    using std::integral_constant;
    if (t.max_verts <= 8 && t.max_faces <= 8)
        launch(integral_constant<uint32_t, 16>{}, integral_constant<uint32_t, 8>{}, dim3((n_queries + 3) / 4));
    else if (t.max_verts <= 16)
        launch(integral_constant<uint32_t, 32>{}, integral_constant<uint32_t, 16>{}, dim3((n_queries + 1) / 2));
    else
        launch(integral_constant<uint32_t, 64>{}, integral_constant<uint32_t, XPBD_MAX_SHAPE_VERTS>{}, dim3(n_queries));
}
} // namespace

hipError_t launch_raycast(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const RayFilter &filter, const void *rays_v, uint32_t n_rays,
                          bool brute, const QueryScratch &s, void *hits_v, hipStream_t stream, const Terrain *terrain, bool terrain_brute)
{
    // the terrain's pass, after the bodies' whichever path that took (null: none, and nothing but the launches below)
    auto finish = [&](hipError_t e) { return e != hipSuccess || !terrain ? e : launch_terrain_rays(*terrain, rays_v, n_rays, terrain_brute, hits_v, stream); };
    if (n_rays == 0)
        return hipSuccess;
    const xpbd_ray *rays = static_cast<const xpbd_ray *>(rays_v);
    xpbd_ray_hit *hits = static_cast<xpbd_ray_hit *>(hits_v);
    launch_query_bodies(b, t, global_id, filter, s, stream);
    if (brute || b.n == 0) {
        const uint32_t tiles = (n_rays + kBruteRays - 1) / kBruteRays, chunks = brute_chunks(b.n, n_rays);
        const uint32_t chunk_len = (b.n + chunks - 1) / chunks;
        Best *partial = static_cast<Best *>(s.brute);
        hipLaunchKernelGGL(k_query_brute, dim3(tiles, chunks), dim3(kBlock), 0, stream, rays, n_rays, b.n, chunk_len, s.rec, b.shape_id,
                           global_id, t, partial);
        hipLaunchKernelGGL(k_query_brute_finish, dim3(n_rays), dim3(64), 0, stream, rays, chunks, partial, s.rec, b.shape_id, t, hits);
        return finish(hipGetLastError());
    }
    if (hipError_t e = launch_query_grid(b, s, stream))
        return e;
    hipLaunchKernelGGL(k_query_walk, dim3(blocks_of(n_rays)), dim3(kBlock), 0, stream, rays, n_rays, b.n, s.rec, b.shape_id, global_id, t,
                       static_cast<QueryGrid *>(s.grid), s.cell_start, s.items, hits);
    return finish(hipGetLastError());
}

QuerySizes overlap_scratch_bytes(uint32_t n, uint32_t n_queries, bool brute)
{
    QuerySizes q = query_scratch_bytes(n, 0, brute || n == 0);
    q.brute = 0;
    const size_t scan = ((size_t)n_queries / 1024 + 8) * 4;
    q.scan_scratch = q.scan_scratch > scan ? q.scan_scratch : scan;
    q.qrec = (size_t)(n_queries ? n_queries : 1) * kOverlapRecDoubles * 8;
    return q;
}

hipError_t launch_overlap(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries_v,
                          uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, uint32_t *offsets, void *hits_v, uint32_t cap,
                          hipStream_t stream, const Terrain *terrain)
{
    if (n_queries == 0)
        return hipMemsetAsync(offsets, 0, sizeof(uint32_t), stream);
    brute = brute || b.n == 0;
    hipError_t e = hipSuccess;
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_overlap_queries, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, static_cast<const xpbd_overlap_query *>(queries_v),
                       n_queries, t, s.qrec);
    if (!brute && (e = launch_query_grid(b, s, stream)) != hipSuccess) // the grid of a ray cast, by the same passes
        return e;
    const OverlapArgs a{pass_args(s, global_id, filter, n_queries, masked, brute), static_cast<const xpbd_overlap_query *>(queries_v), offsets,
                        static_cast<xpbd_overlap_hit *>(hits_v), cap};
    auto pass = [&](auto fill) {
        with_group_shape(t, n_queries, [&](auto l, auto v, dim3 blocks) {
            hipLaunchKernelGGL((k_overlap_pass<decltype(l)::value, decltype(v)::value, decltype(fill)::value>), blocks, dim3(64), 0, stream, b, t, a);
        });
    };
    pass(std::false_type{});
    if (terrain && (e = launch_terrain_overlap(*terrain, t, queries_v, n_queries, false, s.qrec, offsets, hits_v, cap, stream)) != hipSuccess)
        return e;
    if ((e = launch_exclusive_scan(offsets, n_queries, s.scan_scratch, stream)) != hipSuccess)
        return e;
    if (cap) {
        pass(std::true_type{});
        // (before the sort, which takes whole segments: the terrain's index is the largest, so its entry stays the last)
        if (terrain && (e = launch_terrain_overlap(*terrain, t, queries_v, n_queries, true, s.qrec, offsets, hits_v, cap, stream)) != hipSuccess)
            return e;
        if (!brute)
            hipLaunchKernelGGL(k_overlap_sort, dim3(n_queries), dim3(kBlock), 0, stream, offsets, static_cast<xpbd_overlap_hit *>(hits_v), cap);
    }
    return hipGetLastError();
}

hipError_t launch_sweep(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *sweeps_v,
                        uint32_t n_sweeps, bool masked, bool brute, const QueryScratch &s, void *hits_v, hipStream_t stream, const Terrain *terrain,
                        bool terrain_brute)
{
    if (n_sweeps == 0)
        return hipSuccess;
    brute = brute || b.n == 0;
    const xpbd_sweep *sweeps = static_cast<const xpbd_sweep *>(sweeps_v);
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_sweep_queries, dim3(blocks_of(n_sweeps)), dim3(kBlock), 0, stream, sweeps, n_sweeps, t, s.qrec);
    if (!brute)
        if (hipError_t e = launch_query_grid(b, s, stream)) // the grid of a ray cast, by the same passes
            return e;
    const SweepArgs a{pass_args(s, global_id, filter, n_sweeps, masked, brute), sweeps, static_cast<xpbd_sweep_hit *>(hits_v)};
    with_group_shape(t, n_sweeps, [&](auto l, auto v, dim3 blocks) {
        hipLaunchKernelGGL((k_sweep_pass<decltype(l)::value, decltype(v)::value>), blocks, dim3(64), 0, stream, b, t, a);
    });
    const hipError_t e = hipGetLastError();
    return e != hipSuccess || !terrain ? e : launch_terrain_sweeps(*terrain, t, sweeps_v, n_sweeps, terrain_brute, s.qrec, hits_v, stream);
}

hipError_t launch_distance(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries_v,
                           uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, void *hits_v, hipStream_t stream)
{
    if (n_queries == 0)
        return hipSuccess;
    brute = brute || b.n == 0;
    const xpbd_distance_query *queries = static_cast<const xpbd_distance_query *>(queries_v);
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_distance_queries, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, queries, n_queries, t, s.qrec);
    if (!brute)
        if (hipError_t e = launch_query_grid(b, s, stream)) // the grid of a ray cast, by the same passes
            return e;
    const DistanceArgs a{pass_args(s, global_id, filter, n_queries, masked, brute), queries, static_cast<xpbd_distance_hit *>(hits_v)};
    with_group_shape(t, n_queries, [&](auto l, auto v, dim3 blocks) {
        hipLaunchKernelGGL((k_distance_pass<decltype(l)::value, decltype(v)::value>), blocks, dim3(64), 0, stream, b, t, a);
    });
    return hipGetLastError();
}

} // namespace xpbd
