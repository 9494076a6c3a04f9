// xpbd_broadphase.hip -- body-body contact EXTENSION for gfx950: the sphere broadphase on a hashed uniform grid, once per step
// call: bounds and cells, buckets, neighbour lists and the pair list.  Split from xpbd_contacts.hip; declarations and the
// buffers: xpbd_contacts.h.  What it shares with the other units of the pipeline: xpbd_contacts_device.hpp.
//
// Determinism: no floating-point sum is formed here.  Atomics are used on integers only (bucket counts, cursors, the LDS
// cursors of the fill) and every order they leave open is removed by a sort: a body's place in its bucket and a neighbour's
// place in its list are RANKS among distinct ids.  Results do not depend on launch order or on the hash-table size.
#include "xpbd_contacts_device.hpp"
#include "xpbd_scan.h"

namespace xpbd {
namespace {

// Bucket key of a grid cell.  (Tried: a Morton interleave of the coordinates, so that neighbouring cells share cache
// lines.  With equal bits per axis a flat scene -- 144 x 144 x 9 cells -- folds six cells onto one bucket and the
// search slowed down, 178 -> 196 us at 262 144 stacked boxes; the multiplicative hash spreads any extent evenly.)
__device__ __forceinline__ uint32_t cell_hash(int32_t x, int32_t y, int32_t z)
{
    return ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
}

// Bounding sphere of every body: centre = frame * centroid, radius = r_shape + min(|v| dt, r_shape) + pad.
// The clamp keeps one runaway body from inflating the grid cell of everybody (cell edge = 2 * max radius).
// Every workgroup also leaves the largest radius and the bounding box of its centres in c.grid_partials (7 doubles
// per workgroup: no atomics); k_grid reduces them.
__global__ void __launch_bounds__(kBlock) k_bounds(BodyArrays b, PolytopeTables t, const double *__restrict__ shape_radius, double dt,
                                                   double pad, ContactBuffers c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double v[7] = {0.0, DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX}; // rmax, min xyz, max xyz
    if (i < b.n) {
        const uint32_t sid = b.shape_id[i];
        const double *cc = t.centroids + 3 * (size_t)sid;
        const Vec3 centre = body_frame(b, i) * Vec3{cc[0], cc[1], cc[2]};
        const Vec3 vel = load3(b.dyn, D_VEL, b.stride, i);
        const double rs = shape_radius[sid], travel = length(vel) * dt;
        const double r = rs + (travel < rs ? travel : rs) + pad;
        store3(c.centers, 0, b.stride, i, centre);
        c.radius[i] = r;
        v[0] = (r > 0.0 && r <= DBL_MAX) ? r : 0.0;
        const double xyz[3] = {centre.x, centre.y, centre.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) { // a NaN coordinate opens the box completely: the grid then falls back to hashing
            v[1 + a] = xyz[a] == xyz[a] ? xyz[a] : -DBL_MAX;
            v[4 + a] = xyz[a] == xyz[a] ? xyz[a] : DBL_MAX;
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
        c.grid_partials[(size_t)blockIdx.x * 7 + q] = x;
    }
}

__device__ __forceinline__ double clamp_cell(double q)
{
    if (!(q >= -1.0e9)) // NaN or far negative
        q = -1.0e9;
    return q > 1.0e9 ? 1.0e9 : q;
}

// One workgroup: reduces the partials of k_bounds to the grid of this broadphase.  Cell edge = 2 * largest radius, so
// overlapping spheres sit in adjacent cells.  When the box of all centres (plus one cell of margin on every side)
// has no more cells than the table has buckets, the bucket key is the LINEAR cell index (`dense`): neighbouring
// cells are neighbouring buckets, the 27 lookups of a body become 9 runs of 3 consecutive entries and bodies next to
// each other share them.  Otherwise the key is a hash of the cell and buckets may hold several cells.
__global__ void __launch_bounds__(kBlock) k_grid(ContactBuffers c, uint32_t n_partials)
{
    __shared__ double part[kBlock / 64][7];
    double v[7] = {0.0, DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (uint32_t k = threadIdx.x; k < n_partials; k += kBlock)
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const double o = c.grid_partials[(size_t)k * 7 + q];
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
    for (int q = 0; q < 7; ++q)
        for (uint32_t w = 1; w < kBlock / 64; ++w) {
            const double o = part[w][q];
            part[0][q] = (q >= 1 && q <= 3) ? (o < part[0][q] ? o : part[0][q]) : (o > part[0][q] ? o : part[0][q]);
        }
    GridInfo g;
    g.edge = 2.0 * part[0][0];
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = g.edge > 0.0 ? clamp_cell(floor(part[0][1 + a] / g.edge)) : 0.0;
        const double hi = g.edge > 0.0 ? clamp_cell(floor(part[0][4 + a] / g.edge)) : 0.0;
        const double dim = hi >= lo ? hi - lo + 3.0 : 3.0; // one cell of margin on either side
        g.origin[a] = (int32_t)lo - 1;
        g.dims[a] = dim <= 2147483647.0 ? (uint32_t)dim : 0x7FFFFFFFu;
        cells *= dim;
    }
    g.dense = (g.edge > 0.0 && cells <= (double)c.table_size) ? 1u : 0u;
    *c.grid = g;
}

__device__ __forceinline__ uint32_t cell_key(const GridInfo &g, uint32_t table_size, int32_t x, int32_t y, int32_t z)
{
    if (g.dense)
        return (uint32_t)(x - g.origin[0]) + g.dims[0] * ((uint32_t)(y - g.origin[1]) + g.dims[1] * (uint32_t)(z - g.origin[2]));
    return cell_hash(x, y, z) & (table_size - 1);
}

// Grid cell of every body and the population count of its bucket.
__global__ void k_cells(BodyArrays b, ContactBuffers c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const GridInfo g = *c.grid;
    const Vec3 centre = load3(c.centers, 0, b.stride, i);
    int32_t cell[3];
    const double coord[3] = {centre.x, centre.y, centre.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cell[a] = (int32_t)(g.edge > 0.0 ? clamp_cell(floor(coord[a] / g.edge)) : 0.0);
        c.cell[(size_t)a * b.stride + i] = cell[a];
    }
    const uint32_t key = cell_key(g, c.table_size, cell[0], cell[1], cell[2]);
    c.key[i] = key;
    atomicAdd(&c.bucket_start[key], 1u);
}

// The scatter order inside a bucket depends on timing; the bucket's place of body i is instead its RANK among the
// bodies of the bucket (ids are distinct), which every body works out for itself: one lane per body, O(bucket) reads
// each.  (The first version sorted every bucket with one lane and an insertion sort: 55 us per broadphase on the
// mixed scene, whose dense-grid buckets hold ~19 bodies.)
__global__ void k_scatter(BodyArrays b, ContactBuffers c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t key = c.key[i];
    c.items_unsorted[c.bucket_start[key] + atomicAdd(&c.bucket_cursor[key], 1u)] = i;
}

__global__ void k_rank_items(BodyArrays b, ContactBuffers c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t key = c.key[i];
    const uint32_t lo = c.bucket_start[key], hi = c.bucket_start[key + 1];
    uint32_t rank = 0;
    for (uint32_t s = lo; s < hi; ++s)
        rank += c.items_unsorted[s] < i;
    c.items[lo + rank] = i;
}

// Bounding spheres and cells once more, in bucket (slot) order: a bucket scan then reads contiguous memory.
__global__ void k_gather_slots(BodyArrays b, ContactBuffers c)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b.n)
        return;
    const uint32_t j = c.items[s];
    const size_t st = b.stride;
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        c.slot_sphere[a * st + s] = c.centers[a * st + j];
        c.slot_cell[a * st + s] = c.cell[a * st + j];
    }
    c.slot_sphere[3 * st + s] = c.radius[j];
    if (c.filter) { // (a kernel argument: uniform)
        const uint2 f = c.filter[j];
        c.slot_filter[s] = f.x;
        c.slot_filter[st + s] = f.y;
    }
}

// ... and, in a world with sleeping on, who of them is inert.
__global__ void k_gather_slot_inert(BodyArrays b, ContactBuffers c, InertBodies inert)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < b.n)
        inert.slot_inert[s] = inert.inert[c.items[s]];
}

constexpr uint32_t kCellLanes = 8;    // lanes per body in the neighbour kernels
constexpr uint32_t kNbrStage = 128;   // neighbours of one body staged in LDS for the rank sort
constexpr uint32_t kBodiesPerBlock = kBlock / kCellLanes;

// Bucket ranges of the 27 cells around one body, in LDS (one row per body of the block).
struct CellRanges {
    uint32_t start[kBodiesPerBlock][27];
    uint32_t len[kBodiesPerBlock][27];
};

// A joint of the world links i and j.  joint_list holds every joint at both of its ends, so joined(i, j) == joined(j, i).
__device__ __forceinline__ bool joined(const ContactBuffers &c, uint32_t i, uint32_t j)
{
    for (uint32_t k = c.joint_off[i]; k < c.joint_off[i + 1]; ++k) {
        const Joint &jt = c.joints[c.joint_list[k]];
        if ((jt.body_a == i ? jt.body_b : jt.body_a) == j)
            return true;
    }
    return false;
}

// Is body i / the body in slot s inert?  (Without a table: nobody is.)
__device__ __forceinline__ bool inert_body(uint32_t) { return false; }
__device__ __forceinline__ bool inert_body(uint32_t i, const InertBodies &t) { return t.inert[i] != 0; }
__device__ __forceinline__ bool inert_slot(uint32_t) { return false; }
__device__ __forceinline__ bool inert_slot(uint32_t s, const InertBodies &t) { return t.slot_inert[s] != 0; }

// Neighbour search of body i by its group of kCellLanes lanes (`cl` = lane inside the group, `g` = the group's row in
// the LDS tables).  First the 27 bucket ranges are fetched side by side; then the lanes stride over the CONCATENATION
// of the 27 ranges, so every lane has independent loads in flight whatever the occupancy of the single cells.
// Several cells can share a bucket, so a candidate counts only when it sits in the cell being visited: every
// overlapping j != i is visited exactly once, by exactly one lane.  Must be called by all lanes of the block
// (`live` = false for the groups past the last body): it contains a barrier.
// FILTER: a pair whose collision filters exclude each other is no neighbour (the candidate's filter is read in slot order,
// next to its sphere); JOINTED: nor is a pair joined by a joint.  Both tests are symmetric in i and j -- count, fill and
// the pair index of both ends rely on every pair being seen from both of them or from neither.
// inert... (nothing, or the InertBodies of a world with sleeping on): nor is a pair whose two ends are both inert, asleep or
// fixed; one byte per slot, read as the slot's filter is.  Without the argument the two tests are constants and the function
// is what it was before there was one.
template <bool FILTER, bool JOINTED, class Visit, class... Inert>
__device__ __forceinline__ void for_each_neighbour(const BodyArrays &b, const ContactBuffers &c, CellRanges &r, uint32_t i, bool live,
                                                   uint32_t g, uint32_t cl, Visit visit, const Inert &...inert)
{
    const size_t st = b.stride;
    int32_t cx = 0, cy = 0, cz = 0;
    if (live) {
        cx = c.cell[i], cy = c.cell[st + i], cz = c.cell[2 * st + i];
        const GridInfo grid = *c.grid;
        for (uint32_t k = cl; k < 27; k += kCellLanes) {
            const int32_t nx = cx + (int32_t)(k % 3) - 1, ny = cy + (int32_t)((k / 3) % 3) - 1, nz = cz + (int32_t)(k / 9) - 1;
            const uint32_t key = cell_key(grid, c.table_size, nx, ny, nz);
            const uint32_t lo = c.bucket_start[key];
            r.start[g][k] = lo;
            r.len[g][k] = c.bucket_start[key + 1] - lo;
        }
    }
    __syncthreads();
    if (!live)
        return;
    const Vec3 ci = load3(c.centers, 0, b.stride, i);
    const double ri = c.radius[i];
    uint2 fi = {0u, 0u};
    if (FILTER)
        fi = c.filter[i];
    const bool inert_i = inert_body(i, inert...);
    uint32_t k = 0, base = 0; // cell being walked and the position of its first candidate in the concatenation
    for (uint32_t q = cl;; q += kCellLanes) {
        while (k < 27 && q >= base + r.len[g][k])
            base += r.len[g][k++];
        if (k == 27)
            break;
        const uint32_t s = r.start[g][k] + (q - base);
        const int32_t nx = cx + (int32_t)(k % 3) - 1, ny = cy + (int32_t)((k / 3) % 3) - 1, nz = cz + (int32_t)(k / 9) - 1;
        if (c.slot_cell[s] != nx || c.slot_cell[st + s] != ny || c.slot_cell[2 * st + s] != nz)
            continue;
        const uint32_t j = c.items[s];
        if (j == i)
            continue;
        const Vec3 d = ci - load3(c.slot_sphere, 0, b.stride, s);
        const double reach = ri + c.slot_sphere[3 * st + s];
        if (!(dot(d, d) < reach * reach))
            continue;
        if (FILTER && !((fi.x & c.slot_filter[st + s]) && (c.slot_filter[s] & fi.y)))
            continue;
        if (JOINTED && joined(c, i, j))
            continue;
        if (inert_i && inert_slot(s, inert...))
            continue;
        visit(j);
    }
}

__device__ __forceinline__ uint32_t cell_group_sum(uint32_t v)
{
    for (uint32_t off = kCellLanes / 2; off; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// Counts of all neighbours of every body and of those with a larger id.
// (inert...: see for_each_neighbour; the kernels of a world with sleeping on take the table as a third argument)
template <bool FILTER, bool JOINTED, class... Inert>
__global__ void __launch_bounds__(kBlock) k_neighbour_count(BodyArrays b, ContactBuffers c, Inert... inert)
{
    __shared__ CellRanges ranges;
    const uint32_t g = threadIdx.x / kCellLanes, cl = threadIdx.x % kCellLanes;
    // bodies in BUCKET order when the grid is dense (= cell order: the groups of a workgroup then search the same few
    // cells), in index order under the scattering hash (bucket order is a random order there: 178 -> 335 us on `stacks`)
    const uint32_t slot = blockIdx.x * kBodiesPerBlock + g;
    const bool live = slot < b.n;
    const uint32_t i = (live && c.grid->dense) ? c.items[slot] : slot;
    uint32_t all = 0, upper = 0;
    for_each_neighbour<FILTER, JOINTED>(b, c, ranges, i, live, g, cl, [&](uint32_t j) {
        ++all;
        upper += j > i;
    }, inert...);
    if (!live)
        return;
    all = cell_group_sum(all);
    upper = cell_group_sum(upper);
    if (cl == 0) {
        c.nbr_off[i] = all;
        c.pair_first[i] = upper;
    }
}

// Neighbour list of every body, ASCENDING, the pair list i < j in (i, j) order, and upper_start.  The lanes append
// their finds to an LDS list in arrival order; a rank sort (ids are distinct) then gives every entry its final
// place, so the result does not depend on that order.  Lists longer than kNbrStage take a one-lane path.
template <bool FILTER, bool JOINTED, class... Inert>
__global__ void __launch_bounds__(kBlock) k_neighbour_fill(BodyArrays b, ContactBuffers c, Inert... inert)
{
    __shared__ CellRanges ranges;
    __shared__ uint32_t stage[kBodiesPerBlock][kNbrStage];
    __shared__ uint32_t cursor[kBodiesPerBlock];
    const uint32_t g = threadIdx.x / kCellLanes, cl = threadIdx.x % kCellLanes;
    const uint32_t slot = blockIdx.x * kBodiesPerBlock + g;
    const bool live = slot < b.n;
    const uint32_t i = (live && c.grid->dense) ? c.items[slot] : slot;
    uint32_t lo = 0, total = 0;
    if (live) {
        lo = c.nbr_off[i];
        total = c.nbr_off[i + 1] - lo;
    }
    const bool staged = total <= kNbrStage;
    if (cl == 0)
        cursor[g] = 0; // for_each_neighbour's barrier comes before the first visit
    for_each_neighbour<FILTER, JOINTED>(b, c, ranges, i, live, g, cl, [&](uint32_t j) {
        const uint32_t pos = atomicAdd(&cursor[g], 1u);
        if (staged)
            stage[g][pos] = j;
        else
            c.nbr[lo + pos] = j;
    }, inert...);
    __syncthreads();
    if (!live)
        return;
    const uint32_t first = c.pair_first[i];
    if (staged) {
        // entry e of the arrival list goes to place rank(e); lane cl takes e = cl, cl + kCellLanes, ...
        uint32_t below = 0;
        for (uint32_t e = cl; e < total; e += kCellLanes)
            below += stage[g][e] < i;
        below = cell_group_sum(below);
        if (cl == 0)
            c.upper_start[i] = lo + below;
        for (uint32_t e = cl; e < total; e += kCellLanes) {
            const uint32_t v = stage[g][e];
            uint32_t rank = 0;
            for (uint32_t k = 0; k < total; ++k)
                rank += stage[g][k] < v;
            c.nbr[lo + rank] = v;
            if (v > i) {
                const size_t pair = (size_t)first + (rank - below);
                c.pairs[2 * pair] = i;
                c.pairs[2 * pair + 1] = v;
            }
        }
    } else if (cl == 0) {
        for (uint32_t a = lo + 1; a < lo + total; ++a) {
            const uint32_t v = c.nbr[a];
            uint32_t q = a;
            while (q > lo && c.nbr[q - 1] > v) {
                c.nbr[q] = c.nbr[q - 1];
                --q;
            }
            c.nbr[q] = v;
        }
        uint32_t below = 0;
        while (below < total && c.nbr[lo + below] < i)
            ++below;
        c.upper_start[i] = lo + below;
        for (uint32_t k = below; k < total; ++k) {
            c.pairs[2 * (size_t)(first + k - below)] = i;
            c.pairs[2 * (size_t)(first + k - below) + 1] = c.nbr[lo + k];
        }
    }
}

__global__ void k_neighbour_pair_index(BodyArrays b, ContactBuffers c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    for (uint32_t k = c.nbr_off[i]; k < c.nbr_off[i + 1]; ++k) {
        const uint32_t j = c.nbr[k];
        if (j > i) {
            c.nbr_pair[k] = c.pair_first[i] + (k - c.upper_start[i]);
        } else {
            // i sits in the upper part of j's ascending list: binary search
            uint32_t lo = c.upper_start[j], hi = c.nbr_off[j + 1];
            while (lo + 1 < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (c.nbr[mid] <= i)
                    lo = mid;
                else
                    hi = mid;
            }
            c.nbr_pair[k] = c.pair_first[j] + (lo - c.upper_start[j]);
        }
    }
}

// Which form of the neighbour kernels a broadphase runs: bit 0 = group / mask test, bit 1 = jointed-pair test (only when
// there are joints).  A world without filters runs the plain form, the loads of which are those of a world before filters.
// Bit 2 = both-ends-inert test (only with sleeping on): the kernels that take the table.
uint32_t filter_variant(const ContactBuffers &c, const InertBodies &inert)
{
    return (c.filter ? 1u : 0u) | (c.filter_jointed && c.joint_off ? 2u : 0u) | (inert.inert ? 4u : 0u);
}

// The one dispatch of the neighbour kernels: launch(FILTER, JOINTED, table...) with the two flags as std::bool_constant and
// `table...` the InertBodies of a world with sleeping on, or nothing -- the plain forms take no inert argument.
template <class Launch>
void with_neighbour_form(const ContactBuffers &c, const InertBodies &inert, Launch &&launch)
{
    const uint32_t variant = filter_variant(c, inert);
    auto flags = [&](const auto &...table) {
        with_flag(variant & 1u, [&](auto filter) { with_flag(variant & 2u, [&](auto jointed) { launch(filter, jointed, table...); }); });
    };
    if (variant & 4u)
        flags(inert);
    else
        flags();
}

} // namespace

hipError_t launch_bounds_and_cells(const BodyArrays &b, const PolytopeTables &t, const double *shape_radius,
                                   double dt, double pad, const ContactBuffers &c, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(c.bucket_start, 0, (size_t)(c.table_size + 1) * 4, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(c.bucket_cursor, 0, (size_t)c.table_size * 4, stream);
    if (e != hipSuccess || b.n == 0)
        return e;
    hipLaunchKernelGGL(k_bounds, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, t, shape_radius, dt, pad, c);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(kBlock), 0, stream, c, blocks_for(b.n));
    hipLaunchKernelGGL(k_cells, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    return hipGetLastError();
}

hipError_t launch_build_buckets(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert)
{
    hipError_t e = launch_exclusive_scan(c.bucket_start, c.table_size, c.scan_scratch, stream);
    if (e != hipSuccess || b.n == 0)
        return e;
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    hipLaunchKernelGGL(k_rank_items, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    hipLaunchKernelGGL(k_gather_slots, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    if (inert.inert)
        hipLaunchKernelGGL(k_gather_slot_inert, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c, inert);
    return hipGetLastError();
}

hipError_t launch_neighbour_count(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert)
{
    if (b.n) {
        const dim3 grid((b.n + kBodiesPerBlock - 1) / kBodiesPerBlock);
        with_neighbour_form(c, inert, [&](auto filter, auto jointed, const auto &...table) {
            hipLaunchKernelGGL((k_neighbour_count<decltype(filter)::value, decltype(jointed)::value>), grid, dim3(kBlock), 0, stream, b, c,
                               table...);
        });
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = launch_exclusive_scan(c.nbr_off, b.n, c.scan_scratch, stream);
    if (e == hipSuccess)
        e = launch_exclusive_scan(c.pair_first, b.n, c.scan_scratch, stream);
    return e;
}

hipError_t launch_neighbour_fill(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert)
{
    if (b.n == 0)
        return hipSuccess;
    const dim3 grid((b.n + kBodiesPerBlock - 1) / kBodiesPerBlock);
    with_neighbour_form(c, inert, [&](auto filter, auto jointed, const auto &...table) {
        hipLaunchKernelGGL((k_neighbour_fill<decltype(filter)::value, decltype(jointed)::value>), grid, dim3(kBlock), 0, stream, b, c, table...);
    });
    hipLaunchKernelGGL(k_neighbour_pair_index, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    return hipGetLastError();
}

} // namespace xpbd
