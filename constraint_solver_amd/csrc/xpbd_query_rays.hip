// xpbd_query_rays.hip -- scene queries (EXTENSION) for gfx950: batched ray casts against the world's bodies.
//
// Semantics: include/xpbd.h, "Scene queries"; layout of the work: xpbd_query.h.  Determinism: the winner of a ray is the
// minimum of its candidates under one total order -- (t, index) -- and a candidate's t is a function of the ray and the body
// alone, so neither the order in which the atomics of the grid build leave a cell's bodies nor a body being tested in
// several cells changes any bit.  Atomics count integers only.
#include "xpbd_query_units.hpp"

namespace xpbd {
namespace {

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

} // namespace xpbd
