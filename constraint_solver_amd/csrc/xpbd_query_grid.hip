// xpbd_query_grid.hip -- scene queries (EXTENSION) for gfx950: what every family begins with -- the bodies' records
// (k_query_bodies), the uniform grid over their spheres (k_query_grid, k_query_bin) -- and the scratch of a call.
//
// Layout of the work: xpbd_query.h; the routines shared with the families: xpbd_query_device.hpp.  Atomics count integers only.
#include "xpbd_query_units.hpp"

namespace xpbd {
namespace {

uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v)
        p <<= 1;
    return p;
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

QuerySizes overlap_scratch_bytes(uint32_t n, uint32_t n_queries, bool brute)
{
    QuerySizes q = query_scratch_bytes(n, 0, brute || n == 0);
    q.brute = 0;
    const size_t scan = ((size_t)n_queries / 1024 + 8) * 4;
    q.scan_scratch = q.scan_scratch > scan ? q.scan_scratch : scan;
    q.qrec = (size_t)(n_queries ? n_queries : 1) * kOverlapRecDoubles * 8;
    return q;
}

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

} // namespace xpbd
