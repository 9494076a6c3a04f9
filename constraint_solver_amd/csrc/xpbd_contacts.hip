// xpbd_contacts.hip -- body-body contact EXTENSION for gfx950: sphere broadphase on a hashed
// uniform grid and the per-substep contact pipeline
//     integrate + ground contacts  ->  wave-per-pair SAT  ->  Jacobi pair solve + derive.
// Semantics are defined by oracle/xpbd_pairs_oracle.h (op_contacts_step); the reference has no
// body-body contacts, so parity is UNPINNED.  The ground-contact part reuses the reference path
// (xpbd_step.hpp) unchanged.
//
// Determinism: every floating-point sum is formed by ONE lane in a fixed order (neighbour index,
// then manifold point index); atomics are used on integers only (bucket counts, cursors, stats)
// and every order they leave open is removed by a sort.  Results do not depend on launch order,
// on the hash-table size or on how the world is sharded.
#include <cfloat>
#include <type_traits>

#include "xpbd_contacts.h"
#include "xpbd_step.hpp"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
// Worlds up to this many bodies run the pair solve with one lane per manifold POINT (eight lanes per body): below it
// the GPU is not full and a substep costs the dependent chain of one wave, which this shortens.
#ifndef XPBD_SMALL_WORLD
#define XPBD_SMALL_WORLD 16384
#endif
constexpr uint32_t kSmallWorld = XPBD_SMALL_WORLD;
#ifndef XPBD_PAIR_SOLVE_MIN_WAVES
#define XPBD_PAIR_SOLVE_MIN_WAVES 2
#endif

// Bucket key of a grid cell.  (Tried: a Morton interleave of the coordinates, so that neighbouring cells share cache
// lines.  With equal bits per axis a flat scene -- 144 x 144 x 9 cells -- folds six cells onto one bucket and the
// search slowed down, 178 -> 196 us at 262 144 stacked boxes; the multiplicative hash spreads any extent evenly.)
__device__ __forceinline__ uint32_t cell_hash(int32_t x, int32_t y, int32_t z)
{
    return ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
}

// ---------------------------------------------------------------------------------------------------
// Exclusive scan of uint32 (three small kernels; 1024 elements per block).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_scan_exclusive(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wave_sum[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d)
            inc += up;
    }
    if (lane == 63)
        wave_sum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kBlock / 64; ++k) {
        const uint32_t ws = wave_sum[k];
        if (k < wave)
            before += ws;
        all += ws;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ void k_scan_blocks(uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ block_totals)
{
    const uint32_t base = blockIdx.x * (kBlock * 4) + threadIdx.x * 4;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        v[k] = base + k < n ? data[base + k] : 0u;
        sum += v[k];
    }
    uint32_t total;
    uint32_t run = block_scan_exclusive(sum, &total);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (base + k < n)
            data[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0)
        block_totals[blockIdx.x] = total;
}

__global__ void k_scan_totals(uint32_t *__restrict__ block_totals, uint32_t nb)
{
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0)
        carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += kBlock) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < nb ? block_totals[k] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_exclusive(v, &total);
        const uint32_t carry = carry_s;
        if (k < nb)
            block_totals[k] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0)
            carry_s = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        block_totals[nb] = carry_s;
}

__global__ void k_scan_add(uint32_t *__restrict__ data, uint32_t n, const uint32_t *__restrict__ block_totals, uint32_t nb)
{
    const uint32_t base = blockIdx.x * (kBlock * 4) + threadIdx.x * 4;
    const uint32_t add = block_totals[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (base + k < n)
            data[base + k] += add;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        data[n] = block_totals[nb];
}

// ---------------------------------------------------------------------------------------------------
// Broadphase
// ---------------------------------------------------------------------------------------------------
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

// Contact materials (include/xpbd.h, "Contact MATERIALS"): the coefficient of a contact is the smaller of its two sides'.
// (The coefficients are validated on the host: never NaN, so the comparison is an exact minimum.)
__device__ __forceinline__ double min_mu(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double ground_mu(const ContactBuffers &c, uint32_t i) { return min_mu(c.friction[i], c.ground_friction); }

// Body of work item `slot` under a BodySubset (false: nothing to do).
__device__ __forceinline__ bool subset_body(const BodySubset &ss, uint32_t n, uint32_t slot, uint32_t &i)
{
    if (ss.list) {
        if (slot >= ss.count)
            return false;
        i = ss.list[slot];
        return true;
    }
    i = slot;
    return slot < n && !(ss.skip && ss.skip[slot]);
}

// The 13 dynamic doubles of a body as one body-major row (halo buffers): position, rotation s x y z, velocity, angular velocity.
__device__ __forceinline__ void store_row(double *__restrict__ rows, uint32_t r, const BodyDynamic &d)
{
    double *o = rows + (size_t)r * kDynFields;
    o[0] = d.pos.x, o[1] = d.pos.y, o[2] = d.pos.z;
    o[3] = d.rot.s, o[4] = d.rot.x, o[5] = d.rot.y, o[6] = d.rot.z;
    o[7] = d.vel.x, o[8] = d.vel.y, o[9] = d.vel.z;
    o[10] = d.ang.x, o[11] = d.ang.y, o[12] = d.ang.z;
}

__device__ __forceinline__ BodyDynamic load_row(const double *__restrict__ rows, uint32_t r)
{
    const double *o = rows + (size_t)r * kDynFields;
    return BodyDynamic{Vec3{o[0], o[1], o[2]}, Quat{o[3], o[4], o[5], o[6]}, Vec3{o[7], o[8], o[9]}, Vec3{o[10], o[11], o[12]}};
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per body: integrate, remember the frames, ground contacts (reference path).
// ---------------------------------------------------------------------------------------------------
// MATERIALS: the form of a world with contact materials (c.friction set); the plain form never reads them.
// TERRAIN: the form of a world with a heightfield terrain (c.terrain.planes set): the ground contacts of xpbd_step.hpp's terrain forms.
template <bool TRACE, bool MATERIALS, bool TERRAIN = false>
__global__ void __launch_bounds__(kBlock) k_integrate_ground(BodyArrays b, ShapeTable shapes, double h, ContactBuffers c, BodySubset subset,
                                                             uint32_t *__restrict__ last_mask,
                                                             uint32_t *__restrict__ trace_masks, uint32_t trace_row)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_step
    uint32_t *lds_off = reinterpret_cast<uint32_t *>(lds + 3 * shapes.total_verts);
    for (uint32_t k = threadIdx.x; k < 3 * shapes.total_verts; k += blockDim.x)
        lds[k] = shapes.verts[k];
    for (uint32_t k = threadIdx.x; k <= shapes.n_shapes; k += blockDim.x)
        lds_off[k] = shapes.offsets[k];
    __syncthreads();

    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t i;
    if (!subset_body(subset, b.n, slot, i))
        return;
    const uint32_t st = b.stride;
    const BodyStatic s = load_static(b, i);
    // (a ghost body starts the substep from its owner's end-of-substep state, straight from the gathered halo buffer)
    BodyDynamic d = subset.import_buf ? load_row(subset.import_buf, subset.import_rows[slot]) : load_dynamic(b.dyn, st, i);
    const uint32_t sid = b.shape_id[i];
    const uint32_t v0 = lds_off[sid];
    const double compliance = 1e-6 / (h * h);

    const SubstepFrames f = integrate_body(d, s, h);
    uint32_t mask;
    if (TERRAIN)
        mask = solve_ground<MATERIALS, true>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                             c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                             MATERIALS ? ground_mu(c, i) : 0.0, c.terrain);
    else
        mask = solve_ground<MATERIALS>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                       c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                       MATERIALS ? ground_mu(c, i) : 0.0);

    // the pose after the ground contacts lives in the record only: the pair solve (the one reader) takes it from there and
    // rewrites the whole SoA state (velocities come from derive)
    store_record(c.rec, i, f.cur, f.past, d.pos, d.rot, f.past_pos);
    last_mask[i] = mask;
    if (TRACE)
        trace_masks[(size_t)trace_row * st + i] = mask;
}

// ---------------------------------------------------------------------------------------------------
// Heightfield terrain (include/xpbd.h, "TERRAIN"): the plane table, once per xpbd_world_set_terrain, and the sampling call.
// ---------------------------------------------------------------------------------------------------
// One lane per cell: the planes of its lower (h00, h10, h11) and upper (h00, h11, h01) triangle, each {n.x, n.y, n.z, d}, as one
// 64-byte record.  The header's formulas, operation by operation; (double)i is the lookup's floor(u).
__global__ void __launch_bounds__(kBlock) k_terrain_planes(const double *__restrict__ heights, Terrain t, double *__restrict__ planes)
{
    const uint32_t cells_x = t.nx - 1;
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells_x * (t.ny - 1))
        return;
    const uint32_t i = cell % cells_x, j = cell / cells_x;
    const double *row = heights + (size_t)j * t.nx + i;
    const double h00 = row[0], h10 = row[1], h01 = row[t.nx], h11 = row[t.nx + 1];
    const Vec3 corner{t.x0 + (double)i * t.dx, t.y0 + (double)j * t.dy, h00};
    double *out = planes + (size_t)cell * 8;
#pragma unroll
    for (uint32_t upper = 0; upper < 2; ++upper) {
        const double sx = upper ? (h11 - h01) / t.dx : (h10 - h00) / t.dx;
        const double sy = upper ? (h01 - h00) / t.dy : (h11 - h10) / t.dy;
        const Vec3 raw{-sx, -sy, 1.0};
        const Vec3 n = raw * (1.0 / length(raw));
        out[4 * upper + 0] = n.x, out[4 * upper + 1] = n.y, out[4 * upper + 2] = n.z;
        out[4 * upper + 3] = dot(n, corner);
    }
}

// One lane per point: the stepper's lookup at (x, y, 0), then the plane solved for z.
__global__ void __launch_bounds__(kBlock) k_sample_terrain(Terrain t, const double *__restrict__ xy, uint32_t n, double *__restrict__ height,
                                                           double *__restrict__ normal_xyz)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const double x = xy[2 * (size_t)k + 0], y = xy[2 * (size_t)k + 1];
    Plane p;
    double z = __builtin_nan("");
    Vec3 normal{0.0, 0.0, 0.0};
    if (terrain_plane(t, Vec3{x, y, 0.0}, p)) {
        z = (p.displacement - (p.normal.x * x + p.normal.y * y)) / p.normal.z;
        normal = p.normal;
    }
    height[k] = z;
    if (normal_xyz)
        normal_xyz[3 * (size_t)k + 0] = normal.x, normal_xyz[3 * (size_t)k + 1] = normal.y, normal_xyz[3 * (size_t)k + 2] = normal.z;
}

__global__ void k_body_frames(BodyArrays b, double *__restrict__ rec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b.n)
        store_record_p1(rec, i, body_frame(b, i));
}

__global__ void k_stat_records(BodyArrays b, double *__restrict__ stat_rec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t st = b.stride;
    double v[kStatRecDoubles] = {};
    v[0] = b.stat[(size_t)S_INV_MASS * st + i];
    for (uint32_t k = 0; k < 9; ++k)
        v[1 + k] = b.stat[(size_t)(S_INV_INERTIA + k) * st + i];
    for (uint32_t k = 0; k < 3; ++k)
        v[10 + k] = b.stat[(size_t)(S_COM + k) * st + i];
    double2 *r = reinterpret_cast<double2 *>(stat_rec + (size_t)i * kStatRecDoubles);
#pragma unroll
    for (uint32_t k = 0; k < kStatRecDoubles / 2; ++k)
        r[k] = double2{v[2 * k], v[2 * k + 1]};
}

// Rigid::frame() of every body, body-major (7 doubles each), staged through LDS so that the global
// stores are contiguous.
__global__ void __launch_bounds__(kBlock) k_body_frames_aos(BodyArrays b, double *__restrict__ frames)
{
    __shared__ double tile[kBlock * 7];
    const uint32_t base = blockIdx.x * kBlock, i = base + threadIdx.x;
    if (i < b.n) {
        const Frame f = body_frame(b, i);
        double *t = tile + threadIdx.x * 7;
        t[0] = f.position.x, t[1] = f.position.y, t[2] = f.position.z;
        t[3] = f.rotation.s, t[4] = f.rotation.x, t[5] = f.rotation.y, t[6] = f.rotation.z;
    }
    __syncthreads();
    const uint32_t count = min(kBlock, b.n - base);
    for (uint32_t k = threadIdx.x; k < count * 7; k += kBlock)
        frames[(size_t)base * 7 + k] = tile[k];
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per body: Jacobi over the pair contacts, then derive.
// ---------------------------------------------------------------------------------------------------
// What the pair solve needs of a body: pose after the ground contacts, mass properties, and its
// frames before / after this substep's integration.
struct PairBody {
    Vec3 pos;
    Quat rot;
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 com;
    Frame p1, past;
};

// The static fields of body i for its own integrate stage: mass properties from the StatRecord it has loaded anyway, the
// forces and torques (which nobody else reads) from the SoA arrays.
__device__ __forceinline__ BodyStatic static_of(const BodyArrays &b, uint32_t i, double inv_mass, const Mat3 &inv_inertia, Vec3 com)
{
    const uint32_t st = b.stride;
    BodyStatic s;
    s.inv_mass = inv_mass;
    s.inv_inertia = inv_inertia;
    s.com = com;
    s.ext_force = load3(b.stat, S_EXT_FORCE, st, i);
    s.int_force = load3(b.stat, S_INT_FORCE, st, i);
    s.ext_torque = load3(b.stat, S_EXT_TORQUE, st, i);
    s.int_torque = load3(b.stat, S_INT_TORQUE, st, i);
    return s;
}

// The BodyRecords of a workgroup's OWN bodies, staged in LDS (the per-body kernels with one lane per body and no body list):
// a body's neighbours are gathers of whole records -- 2 x 128-byte lines each -- and in an index-coherent scene (box stacks: a
// column is 16 consecutive bodies) most of them are bodies of the same workgroup, whose records the workgroup has loaded once
// already.  PMC on `stacks` (profiles/r02_c): 373 MB read per launch for ~160 MB of distinct data, the kernel at the gather
// rate of the memory system (5.3 TB/s of lines).  Word k of the record of the workgroup's body t sits at words[k * kBlock + t]:
// consecutive lanes read consecutive 16-byte words (no bank conflicts).  Same values from another place: same bits.
#ifndef XPBD_PAIR_SOLVE_STAGE_RECORDS
#define XPBD_PAIR_SOLVE_STAGE_RECORDS 0 // measured and rejected, see DESIGN.md 8 (the fetched bytes of the kernel fall by 29 % on box stacks, its time does not)
#endif
struct RecordStage {
    const double2 *words = nullptr; // LDS; null = not staged
    uint32_t first = 0, count = 0;  // bodies [first, first + count) are staged
};

__device__ __forceinline__ BodyRecord load_record_staged(const double *__restrict__ rec, uint32_t i, const RecordStage &stage)
{
    const uint32_t t = i - stage.first;
    if (stage.words && t < stage.count) {
        double2 v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            v[k] = stage.words[k * kBlock + t];
        BodyRecord o;
        o.p1 = Frame{Vec3{v[0].x, v[0].y, v[1].x}, Quat{v[1].y, v[2].x, v[2].y, v[3].x}};
        o.past = Frame{Vec3{v[3].y, v[4].x, v[4].y}, Quat{v[5].x, v[5].y, v[6].x, v[6].y}};
        o.pos = Vec3{v[7].x, v[7].y, v[8].x};
        o.rot = Quat{v[8].y, v[9].x, v[9].y, v[10].x};
        o.past_pos = Vec3{v[10].y, v[11].x, v[11].y};
        return o;
    }
    return load_record(rec, i);
}

// Every thread of the workgroup calls this (it ends in a barrier): thread t stages the record of body `first + t`.
__device__ __forceinline__ RecordStage stage_records(double2 *__restrict__ words, const double *__restrict__ rec, uint32_t first, uint32_t n)
{
    const uint32_t t = threadIdx.x, i = first + t;
    if (i < n) {
        const double2 *r = reinterpret_cast<const double2 *>(rec + (size_t)i * kRecDoubles);
        double2 v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            v[k] = r[k];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            words[k * kBlock + t] = v[k];
    }
    __syncthreads();
    RecordStage s;
    s.words = words;
    s.first = first;
    s.count = n > first ? (n - first < kBlock ? n - first : kBlock) : 0u;
    return s;
}

// (past_pos: optional, the position before integrate -- only a body's own derive needs it)
__device__ __forceinline__ PairBody load_pair_body(const ContactBuffers &c, uint32_t i, Vec3 *past_pos = nullptr,
                                                   const RecordStage &stage = RecordStage())
{
    const BodyRecord r = load_record_staged(c.rec, i, stage); // two cache lines, or LDS
    const StatRecord s = load_stat_record(c.stat_rec, c.stat_index ? c.stat_index[i] : i); // one, or a cached table entry
    PairBody p;
    p.pos = r.pos;
    p.rot = r.rot;
    p.inv_mass = s.inv_mass;
    p.inv_inertia = s.inv_inertia;
    p.com = s.com;
    p.p1 = r.p1;
    p.past = r.past;
    if (past_pos)
        *past_pos = r.past_pos;
    return p;
}

// Frame::delta, src/frame.rs:40-44
__device__ __forceinline__ Vec3 frame_delta(const Frame &cur, const Frame &past, Vec3 global)
{
    const Vec3 local = inverse(cur) * global;
    return global - past * local;
}

// Constraint::inverse_resitance for one body, src/constraint.rs:25-32
// (Body: PairBody -- the pose after the ground contacts -- or the velocity pass's VelBody, the pose after derive)
template <class Body>
__device__ __forceinline__ double generalized_inverse_mass(const Body &p, Vec3 point, Vec3 dir)
{
    const Vec3 angular_impulse = conjugate(p.rot) * cross(point - (p.pos + p.com), dir);
    return p.inv_mass + dot(p.inv_inertia * angular_impulse, angular_impulse);
}

// The angular limits of joint `joint` for body `self` (xpbd.h, XPBD_LIMIT_*): every limit that binds is a Jacobi entry of its
// own, in the caller's order.  Evaluated per body like the hinge's angular term, 3-vectors selected by role (a / b), so both
// ends of the joint compute the same phi, n and lambda.  A limit that does not bind adds nothing, not even to `count`.
#ifndef XPBD_JOINT_LIMIT_INLINE
#define XPBD_JOINT_LIMIT_INLINE __forceinline__
#endif
__device__ XPBD_JOINT_LIMIT_INLINE void joint_limit_terms(const ContactBuffers &c, uint32_t joint, const Joint &jt, bool self_is_a,
                                                          const PairBody &self, const PairBody &other, double compliance, Quat &drot,
                                                          uint32_t &count)
{
    const uint32_t l_end = c.limit_off[joint + 1];
    for (uint32_t l = c.limit_off[joint]; l < l_end; ++l) {
        const JointLimit &lim = c.limits[l];
        const Quat q_a = self_is_a ? self.rot : other.rot, q_b = self_is_a ? other.rot : self.rot;
        const Vec3 a_w = q_a * Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
        double phi;
        Vec3 n;
        if (lim.kind == XPBD_LIMIT_SWING) {
            const Vec3 b_w = q_b * Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
            const Vec3 cr = cross(a_w, b_w);
            const double s = length(cr);
            if (s == 0.0)
                continue;
            phi = atan2(s, dot(a_w, b_w));
            n = cr * (1.0 / s);
        } else {
            Vec3 p_a = q_a * Vec3{lim.ref_a[0], lim.ref_a[1], lim.ref_a[2]};
            Vec3 p_b = q_b * Vec3{lim.ref_b[0], lim.ref_b[1], lim.ref_b[2]};
            if (lim.kind == XPBD_LIMIT_HINGE) {
                n = a_w;
            } else { // XPBD_LIMIT_TWIST: about the bisector of the two axes, on the references' projections
                const Vec3 bisector = a_w + q_b * Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
                const double len = length(bisector);
                if (len == 0.0)
                    continue;
                n = bisector * (1.0 / len);
                p_a = p_a - n * dot(p_a, n);
                p_b = p_b - n * dot(p_b, n);
            }
            phi = atan2(dot(cross(p_a, p_b), n), dot(p_a, p_b));
        }
        const double clamped = phi < lim.lower ? lim.lower : (phi > lim.upper ? lim.upper : phi);
        const double err = phi - clamped;
        if (err == 0.0)
            continue;
        const Vec3 n_self = conjugate(self.rot) * n, n_other = conjugate(other.rot) * n;
        const double w_s = dot(self.inv_inertia * n_self, n_self), w_o = dot(other.inv_inertia * n_other, n_other);
        const double w = self_is_a ? w_s + w_o : w_o + w_s; // w_a + w_b
        const double lambda = err / (w + compliance);
        const Vec3 turn = self_is_a ? lambda * n : (-lambda) * n;
        const Quat spin = quat_sv(0.0, self.inv_inertia * turn);
        drot = drot + (0.5 * spin) * self.rot;
        ++count;
    }
}

// Jacobi pair solve + joints + derive of body i: its state at the end of the substep.
// (touching, points: += the manifolds with contact points among this body's pairs (i, j > i) and their points -- every
// pair is counted by its smaller body, which gives the pipeline's statistics without a pass of their own)
//
// G = lanes per body.  G = 1: the lane walks the points of a manifold one after the other.  G = 8 (small worlds, where
// a wave's dependent chain is the whole cost): lane `sub` evaluates point `sub` of the manifold, and the terms are then
// added on every lane in point order -- the same values in the same order, so the same bits.
#ifndef XPBD_PAIR_SOLVE_ROUND_POINTS
#define XPBD_PAIR_SOLVE_ROUND_POINTS 2 // points of a manifold per round, see pass 2 below; A/B (boxes pile / mixed pile SAT / GJK+EPA,
                                       // 1e8 body-substeps/s): 1 point 5.24 / 2.56 / 2.76, 2 points 5.35 / 2.57 / 2.80, 3 points 5.30 / 2.54 / 2.75
#endif
// MATERIALS: contact materials are set (c.friction; uniform over the launch, chosen by the launcher).  The plain form is the
// reference's contact: it loads no coefficient and keeps the literal 1.0.
template <uint32_t G, bool MATERIALS>
__device__ __forceinline__ BodyDynamic pair_solve_derive_body(const ContactBuffers &c, uint32_t i, double h,
                                                              const PairBody &self, Vec3 self_past_pos, uint32_t sub, uint32_t &touching,
                                                              uint32_t &points, const RecordStage &stage = RecordStage())
{
    static_assert(G == 1 || G == kMaxManifoldPoints, "one lane per body or one lane per manifold point");
    const double compliance = 1e-6 / (h * h);
    const double limit = c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0;
    const double mu_self = MATERIALS ? c.friction[i] : 0.0;

    Vec3 dpos{0.0, 0.0, 0.0};
    Quat drot{0.0, 0.0, 0.0, 0.0};
    uint32_t count = 0;
    // One neighbour with contact points: its points' terms added in point order.
    auto neighbour_terms = [&](uint32_t j, const ContactManifold *m, uint32_t n_points, uint32_t feature, uint32_t pt_begin, uint32_t pt_end) {
        if (j > i && pt_begin == 0) {
            ++touching;
            points += n_points;
        }
        const PairBody other = load_pair_body(c, j, nullptr, stage);
        const double mu = MATERIALS ? min_mu(mu_self, c.friction[j]) : 0.0; // (only touching neighbours get here)
        // pair (A, B) = (min, max); the reference body is A unless the reference face is on B.  The formulas are
        // written in terms of the incident and the reference body; here every term is evaluated for `self` and
        // `other` with their own point and only 3-vectors are selected by role -- selecting whole bodies by a
        // per-lane condition made the compiler keep four body records live (255 VGPRs + AGPRs, one wave per SIMD).
        const bool self_is_a = i < j;
        const bool ref_is_a = feature != 1u;
        const bool self_is_inc = self_is_a != ref_is_a;
        // a face contact stores its reference plane and the points on the incident body; their partners on the reference
        // body are the clipper's projections, re-evaluated with its own expression (xpbd_clip.hpp: Plane::project) -- the
        // same inputs through the same operations, so the same bits.  Feature 2: the single contact's two points.
        const bool face = feature != 2u;
        const Plane ref_plane{Vec3{m->plane[0], m->plane[1], m->plane[2]}, m->plane[3]};
        // one contact point: what it adds to dpos and drot
        auto point_term = [&](uint32_t pt, Vec3 &term_pos, Quat &term_rot) {
            const Vec3 p_inc{m->point[pt][0], m->point[pt][1], m->point[pt][2]};
            Vec3 p_ref;
            if (face) {
                const double depth = distance(ref_plane, p_inc);
                p_ref = p_inc - depth * ref_plane.normal;
            } else {
                p_ref = Vec3{m->point[1][0], m->point[1][1], m->point[1][2]};
            }
            const Vec3 p_self = self_is_inc ? p_inc : p_ref, p_other = self_is_inc ? p_ref : p_inc;
            const Vec3 correction = p_ref - p_inc;
            const Vec3 moved_self = frame_delta(self.p1, self.past, p_self), moved_other = frame_delta(other.p1, other.past, p_other);
            const Vec3 delta_rel = self_is_inc ? moved_self - moved_other : moved_other - moved_self; // incident - reference
            const Vec3 delta_tangential = delta_rel - project_on(delta_rel, correction);
            const Vec3 c0 = p_inc;
            double k = 1.0;
            if (MATERIALS) { // Coulomb's cone on positions: at most mu * |correction| of the tangential slip is taken back
                const double bound = mu * length(correction);
                const double len_t = length(delta_tangential);
                if (bound < len_t) // (false for mu = +inf, a NaN bound, len_t = 0: the reference's contact)
                    k = bound / len_t;
            }
            const Vec3 c1 = p_ref - k * delta_tangential;
            const Vec3 difference = c1 - c0;
            const double dist = length(difference);
            const Vec3 dir = difference * (1.0 / dist);
            // w = w_incident + w_reference; IEEE addition commutes, so the order of the two bodies does not matter
            const double w = generalized_inverse_mass(self, p_self, dir) + generalized_inverse_mass(other, p_other, dir);
            double error = dist;
            if (limit > 0.0) { // xpbd_world_set_max_depenetration_speed (uniform over the launch; 0 = off); oracle: accumulate_point
                const double len = length(correction);
                const double closing = len > 0.0 ? dot(delta_rel, correction) / len : 0.0;
                double allowed = limit - closing;
                if (!(allowed > 0.0))
                    allowed = 0.0;
                if (dist > allowed)
                    error = allowed;
            }
            const double lambda = (error - 0.0) / (w + compliance);

            const Vec3 impulse = self_is_inc ? lambda * dir : (-lambda) * dir;
            term_pos = impulse * self.inv_mass;
            const Vec3 arm = p_self - (self.pos + self.com);
            const Quat spin = quat_sv(0.0, cross(self.inv_inertia * arm, impulse));
            term_rot = (0.5 * spin) * self.rot;
        };
        if (G == 1) {
            for (uint32_t pt = pt_begin; pt < pt_end; ++pt) {
                Vec3 term_pos;
                Quat term_rot;
                point_term(pt, term_pos, term_rot);
                dpos = dpos + term_pos;
                drot = drot + term_rot;
                ++count;
            }
        } else {
            Vec3 term_pos{0.0, 0.0, 0.0};
            Quat term_rot{0.0, 0.0, 0.0, 0.0};
            if (sub < n_points)
                point_term(sub, term_pos, term_rot);
            for (uint32_t pt = 0; pt < n_points; ++pt) { // every lane of the group adds the terms in point order
                dpos = dpos + Vec3{__shfl(term_pos.x, pt, G), __shfl(term_pos.y, pt, G), __shfl(term_pos.z, pt, G)};
                drot = drot + Quat{__shfl(term_rot.s, pt, G), __shfl(term_rot.x, pt, G), __shfl(term_rot.y, pt, G),
                                   __shfl(term_rot.z, pt, G)};
                ++count;
            }
        }
    };
    // Pass 1 -- which of the body's neighbour slots have contact points: bit u of `touch` = slot k_begin + u.  The
    // neighbours in batches of four: their pair indices, then their point counts, are fetched side by side, so a body
    // pays two dependent round trips per batch instead of two per neighbour (most neighbours of a loose scene do not
    // touch, and the whole cost of looking at them is that latency).
    // Pass 2 -- the lanes of a wave then walk THEIR OWN touching neighbours, round by round (ascending, so every body
    // still adds its terms in the oracle's order): a wave runs as many rounds as its busiest body has touching
    // neighbours.  Walking the slots in lockstep instead made it run every slot that any of its 64 bodies had a
    // contact in -- in a settled pile of boxes (7.8 neighbours a body, 3.2 of them touching) 14 slots with four lanes in
    // ten idle in each: 17 % lane utilisation (PMC), 19 000 VALU instructions per wave.
    const uint32_t k_end = c.nbr_off[i + 1];
    for (uint32_t k_base = c.nbr_off[i]; k_base < k_end; k_base += 64) { // (64 slots per mask: one trip for all but monsters)
        const uint32_t k_stop = k_end - k_base > 64u ? k_base + 64u : k_end;
        unsigned long long touch = 0;
        // (a wave whose bodies all have one or two neighbours -- box stacks -- skips pass 1: nothing to filter there)
        const bool few = __all(k_stop - k_base <= 2u);
        if (few)
            touch = k_stop - k_base == 2u ? 3ull : 1ull;
        for (uint32_t k0 = k_base; !few && k0 < k_stop; k0 += 4) {
            uint32_t pair_of[4], points_of[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                pair_of[u] = k0 + u < k_stop ? c.nbr_pair[k0 + u] : 0u;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                points_of[u] = k0 + u < k_stop ? (uint32_t)c.pair_codes[pair_of[u]] : 0u;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                if (points_of[u])
                    touch |= 1ull << (k0 - k_base + u);
        }
        // (the next neighbour and its pair index are fetched while the current one's points are evaluated)
        uint32_t j_next = 0, pair_next = 0;
        if (touch) {
            const uint32_t k = k_base + (uint32_t)__ffsll((long long)touch) - 1u;
            j_next = c.nbr[k], pair_next = c.nbr_pair[k];
        }
        // A round takes at most `chunk` points of a manifold; a longer manifold goes on in the lane's next round.  The
        // rounds of a wave are as long as their longest share, and in a pile the manifolds have 1.4 points on average but
        // four in the longest: with whole manifolds per round the lanes idled through two thirds of every round (PMC:
        // 26 % lane utilisation).  Stacks (every manifold four points) take them whole.  G lanes per body: one point per lane.
        const uint32_t chunk = (G > 1 || few) ? kMaxManifoldPoints : (uint32_t)XPBD_PAIR_SOLVE_ROUND_POINTS;
        uint32_t j_cur = 0, pair_cur = 0, code_cur = 0, n_cur = 0, pt = 0;
        while (touch || pt < n_cur) {
            if (pt == n_cur) { // this lane's next touching neighbour
                j_cur = j_next, pair_cur = pair_next;
                touch &= touch - 1ull;
                if (touch) {
                    const uint32_t k = k_base + (uint32_t)__ffsll((long long)touch) - 1u;
                    j_next = c.nbr[k], pair_next = c.nbr_pair[k];
                }
                code_cur = c.pair_codes[pair_cur];
                n_cur = code_cur & ((1u << kPairCodeFeatureShift) - 1u);
                pt = 0;
            }
            if (n_cur) { // (zero only after the shortcut above: a listed neighbour that does not touch)
                const uint32_t stop = n_cur - pt > chunk ? pt + chunk : n_cur;
                neighbour_terms(j_cur, c.manifolds + pair_cur, n_cur, code_cur >> kPairCodeFeatureShift, pt, stop);
                pt = stop;
            }
        }
    }

    // joints of this body, ascending joint index (same accumulator: the "mixed-constraint" pass)
    if (c.joint_off) {
        for (uint32_t k = c.joint_off[i]; k < c.joint_off[i + 1]; ++k) {
            const Joint &jt = c.joints[c.joint_list[k]];
            const bool self_is_a = jt.body_a == i;
            const PairBody other = load_pair_body(c, self_is_a ? jt.body_b : jt.body_a, nullptr, stage);
            // as above: evaluate per body, select 3-vectors by role (a / b)
            const Vec3 anchor_self = self_is_a ? Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]} : Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]};
            const Vec3 anchor_other = self_is_a ? Vec3{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]} : Vec3{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]};
            const Vec3 p_self = Frame{frame_origin(self.pos, self.rot, self.com), self.rot} * anchor_self;
            const Vec3 p_other = Frame{frame_origin(other.pos, other.rot, other.com), other.rot} * anchor_other;
            const Vec3 difference = self_is_a ? p_other - p_self : p_self - p_other; // p_b - p_a
            const double dist = length(difference);
            // (coincident points: the reference's direction() would be NaN (K6); nothing to correct.  A slider has no
            // positional term: its anchor is held to the axis by k_joint_extras)
            if (dist != 0.0 && jt.kind != XPBD_JOINT_SLIDER) {
                const Vec3 dir = difference * (1.0 / dist);
                const double w = generalized_inverse_mass(self, p_self, dir) + generalized_inverse_mass(other, p_other, dir);
                const double lambda = (dist - jt.distance) / (w + compliance);
                const Vec3 impulse = self_is_a ? lambda * dir : (-lambda) * dir;
                dpos = dpos + impulse * self.inv_mass;
                const Vec3 arm = p_self - (self.pos + self.com);
                const Quat spin = quat_sv(0.0, cross(self.inv_inertia * arm, impulse));
                drot = drot + (0.5 * spin) * self.rot;
                ++count;
            }
            if (jt.kind != XPBD_JOINT_DISTANCE) { // XPBD_JOINT_HINGE, XPBD_JOINT_SLIDER
                // the angular term (oracle: accumulate_hinge): the joint's axes, unit vectors in the object space of a and b,
                // are kept aligned; evaluated per body, 3-vectors selected by role as above
                const Vec3 axis_self = self_is_a ? Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]} : Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]};
                const Vec3 axis_other = self_is_a ? Vec3{jt.axis_b[0], jt.axis_b[1], jt.axis_b[2]} : Vec3{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
                const Vec3 w_self = self.rot * axis_self, w_other = other.rot * axis_other;
                const Vec3 delta = self_is_a ? cross(w_self, w_other) : cross(w_other, w_self); // a_w x b_w
                const double mag = length(delta);
                if (mag != 0.0) {
                    const Vec3 n = delta * (1.0 / mag);
                    const Vec3 n_self = conjugate(self.rot) * n, n_other = conjugate(other.rot) * n;
                    const double w_s = dot(self.inv_inertia * n_self, n_self), w_o = dot(other.inv_inertia * n_other, n_other);
                    const double w = self_is_a ? w_s + w_o : w_o + w_s; // w_a + w_b (IEEE addition commutes; written out for the reader)
                    const double lambda = mag / (w + compliance);
                    const Vec3 turn = self_is_a ? lambda * n : (-lambda) * n;
                    const Quat spin = quat_sv(0.0, self.inv_inertia * turn);
                    drot = drot + (0.5 * spin) * self.rot;
                    ++count;
                }
            }
            if (c.limit_off)
                joint_limit_terms(c, c.joint_list[k], jt, self_is_a, self, other, compliance, drot, count);
            if (c.joint_extra) { // the joint's extra entries for this end, summed by k_joint_extras into the record of this
                                 // slot of the body's joint list (zero count: none; adding zeros could flip the sign of a zero)
                const double *e = c.joint_extra + (size_t)k * kJointExtraDoubles;
                if (e[7] != 0.0) {
                    dpos = dpos + Vec3{e[0], e[1], e[2]};
                    drot = drot + Quat{e[3], e[4], e[5], e[6]};
                    count += (uint32_t)e[7];
                }
            }
        }
    }

    BodyDynamic d;
    d.pos = self.pos;
    d.rot = self.rot;
    if (count) {
        const double cnt = (double)count;
        d.pos = self.pos + dpos / cnt;
        d.rot = normalized(self.rot + Quat{drot.s / cnt, drot.x / cnt, drot.y / cnt, drot.z / cnt});
    }
    derive_body(d, self_past_pos, self.past.rotation, h);
    return d;
}

// stats[0] += touching, stats[1] += points, summed over the workgroup: TWO atomics per workgroup (same-address atomics
// serialise at ~10-25 ns each -- never one per pair, see xpbd_pairs.hip).  Every thread of the block must call this.
__device__ __forceinline__ void block_add_stats(uint32_t touching, uint32_t points, unsigned long long *__restrict__ stats)
{
    for (uint32_t off = 32; off; off >>= 1) {
        touching += __shfl_xor(touching, off, 64);
        points += __shfl_xor(points, off, 64);
    }
    __shared__ uint32_t part[2][kBlock / 64];
    if ((threadIdx.x & 63u) == 0) {
        part[0][threadIdx.x >> 6] = touching;
        part[1][threadIdx.x >> 6] = points;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0, p = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            t += part[0][w];
            p += part[1][w];
        }
        if (t)
            atomicAdd(&stats[0], (unsigned long long)t);
        if (p)
            atomicAdd(&stats[1], (unsigned long long)p);
    }
}

template <uint32_t G, bool MATERIALS>
__global__ void __launch_bounds__(kBlock, XPBD_PAIR_SOLVE_MIN_WAVES) k_pair_solve_derive(BodyArrays b, double *__restrict__ dyn_out, double h,
                                                                                        ContactBuffers c, BodySubset subset)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, slot = gid / G, sub = gid % G;
    // one lane per body, bodies in index order: the workgroup's own records go through LDS (load_record_staged)
    constexpr bool kStage = G == 1 && XPBD_PAIR_SOLVE_STAGE_RECORDS;
    __shared__ double2 stage_words[kStage ? 12 * kBlock : 1];
    RecordStage stage;
    if (kStage && !subset.list)
        stage = stage_records(stage_words, c.rec, blockIdx.x * kBlock, b.n);
    uint32_t touching = 0, points = 0, i;
    if (subset_body(subset, b.n, slot, i)) {
        Vec3 past_pos;
        const PairBody self = load_pair_body(c, i, &past_pos, stage);
        const BodyDynamic d = pair_solve_derive_body<G, MATERIALS>(c, i, h, self, past_pos, sub, touching, points, stage);
        if (sub == 0) {
            store_dynamic(dyn_out, b.stride, i, d);
            if (subset.export_rows)
                store_row(subset.export_rows, slot, d);
        }
    }
    block_add_stats(sub == 0 ? touching : 0u, sub == 0 ? points : 0u, c.stats);
}

// The end of substep k and the beginning of substep k + 1 of one body in one kernel: pair solve + derive, then
// integrate + ground contacts straight from registers.  Nothing a body needs from the others changes in between
// (they read each other's state of substep k: dyn and the frames of `c`), so the new state goes to the other dyn
// buffer and the frames of substep k + 1 to the other frame set (`next`).  Saves the store + reload of the dynamic
// state, half of the static loads and one launch per substep; same arithmetic, same bits.  Only for step calls
// that run all their substeps on one device: a halo exchange sits exactly at this seam.
// (G lanes per body as in pair_solve_derive_body; with G = 8 the integrate + ground part runs redundantly on the eight
// lanes and lane 0 stores.)
template <bool TRACE, uint32_t G, bool MATERIALS>
__global__ void __launch_bounds__(kBlock, XPBD_PAIR_SOLVE_MIN_WAVES) k_pair_solve_integrate_ground(
    BodyArrays b, ShapeTable shapes, double h, ContactBuffers c, BodySubset subset, double *__restrict__ next_rec,
    uint32_t *__restrict__ last_mask, uint32_t *__restrict__ trace_masks, uint32_t trace_row)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_integrate_ground
    uint32_t *lds_off = reinterpret_cast<uint32_t *>(lds + 3 * shapes.total_verts);
    for (uint32_t k = threadIdx.x; k < 3 * shapes.total_verts; k += blockDim.x)
        lds[k] = shapes.verts[k];
    for (uint32_t k = threadIdx.x; k <= shapes.n_shapes; k += blockDim.x)
        lds_off[k] = shapes.offsets[k];
    __syncthreads();

    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, slot = gid / G, sub = gid % G;
    constexpr bool kStage = G == 1 && XPBD_PAIR_SOLVE_STAGE_RECORDS; // see k_pair_solve_derive
    __shared__ double2 stage_words[kStage ? 12 * kBlock : 1];
    RecordStage stage;
    if (kStage && !subset.list)
        stage = stage_records(stage_words, c.rec, blockIdx.x * kBlock, b.n);
    uint32_t touching = 0, points = 0, i;
    if (subset_body(subset, b.n, slot, i)) {
        const uint32_t st = b.stride;
        BodyDynamic d;
        BodyStatic s;
        {
            Vec3 past_pos;
            const PairBody self = load_pair_body(c, i, &past_pos, stage);
            d = pair_solve_derive_body<G, MATERIALS>(c, i, h, self, past_pos, sub, touching, points, stage);
            s = static_of(b, i, self.inv_mass, self.inv_inertia, self.com);
        }
        if (subset.export_rows && sub == 0)
            store_row(subset.export_rows, slot, d); // the end-of-substep state, before the next substep's integration
        const uint32_t sid = b.shape_id[i];
        const uint32_t v0 = lds_off[sid];
        const double compliance = 1e-6 / (h * h);
        const SubstepFrames f = integrate_body(d, s, h);
        const uint32_t mask = solve_ground<MATERIALS>(d, s, f, compliance, lds + 3 * v0, lds_off[sid + 1] - v0,
                                                      c.max_depenetration_speed > 0.0 ? c.max_depenetration_speed * h : 0.0,
                                                      MATERIALS ? ground_mu(c, i) : 0.0);
        if (sub == 0) {
            // everything the next kernel needs of this body is its record: no SoA state is written between the substeps of
            // a step call (the last substep's k_pair_solve_derive writes all 13 dynamic fields)
            store_record(next_rec, i, f.cur, f.past, d.pos, d.rot, f.past_pos);
            last_mask[i] = mask;
            if (TRACE)
                trace_masks[(size_t)trace_row * st + i] = mask;
        }
    }
    block_add_stats(sub == 0 ? touching : 0u, sub == 0 ? points : 0u, c.stats);
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per joint with extras: sliders and joint drives (include/xpbd.h, "SLIDERS and joint DRIVES").
// ---------------------------------------------------------------------------------------------------
// The summed extra entries of one joint end.
struct ExtraSum {
    Vec3 dpos{0.0, 0.0, 0.0};
    Quat drot{0.0, 0.0, 0.0, 0.0};
    uint32_t count = 0;
};

// One linear entry: the impulse +lambda n on a at p_a, -lambda n on b at p_b, applied as the positional term applies its own.
__device__ __forceinline__ void extra_linear_entry(const PairBody &a, const PairBody &b, Vec3 p_a, Vec3 p_b, Vec3 n, double lambda, ExtraSum &sum_a,
                                                   ExtraSum &sum_b)
{
    const Vec3 impulse_a = lambda * n, impulse_b = (-lambda) * n;
    sum_a.dpos = sum_a.dpos + impulse_a * a.inv_mass;
    sum_b.dpos = sum_b.dpos + impulse_b * b.inv_mass;
    const Vec3 arm_a = p_a - (a.pos + a.com), arm_b = p_b - (b.pos + b.com);
    const Quat spin_a = quat_sv(0.0, cross(a.inv_inertia * arm_a, impulse_a)), spin_b = quat_sv(0.0, cross(b.inv_inertia * arm_b, impulse_b));
    sum_a.drot = sum_a.drot + (0.5 * spin_a) * a.rot;
    sum_b.drot = sum_b.drot + (0.5 * spin_b) * b.rot;
    ++sum_a.count;
    ++sum_b.count;
}

// One angular entry: a turns by +lambda n, b by -lambda n, as a limit's entry does.
__device__ __forceinline__ void extra_angular_entry(const PairBody &a, const PairBody &b, Vec3 n, double lambda, ExtraSum &sum_a, ExtraSum &sum_b)
{
    const Quat spin_a = quat_sv(0.0, a.inv_inertia * (lambda * n)), spin_b = quat_sv(0.0, b.inv_inertia * ((-lambda) * n));
    sum_a.drot = sum_a.drot + (0.5 * spin_a) * a.rot;
    sum_b.drot = sum_b.drot + (0.5 * spin_b) * b.rot;
    ++sum_a.count;
    ++sum_b.count;
}

__device__ __forceinline__ double wrap_angle(double x)
{
    const double pi = 3.14159265358979323846;
    return x > pi ? x - 2.0 * pi : (x < -pi ? x + 2.0 * pi : x);
}

__device__ __forceinline__ void store_extra_sum(double *__restrict__ out, const ExtraSum &s)
{
    double2 *o = reinterpret_cast<double2 *>(out);
    o[0] = double2{s.dpos.x, s.dpos.y};
    o[1] = double2{s.dpos.z, s.drot.s};
    o[2] = double2{s.drot.x, s.drot.y};
    o[3] = double2{s.drot.z, (double)s.count};
}

// One lane per joint with extras.  Both ends are loaded from the records of this substep and every term is evaluated ONCE,
// so both ends get the same phi, n and lambda; the two sums go to the records of the joint's two slots in the bodies' joint
// lists (c.extra_slots), where the pair solve of the same substep picks them up.  Nothing here is read by another lane of the launch.
__global__ void __launch_bounds__(kBlock) k_joint_extras(double h, ContactBuffers c)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= c.n_extra_joints)
        return;
    const uint32_t joint = c.extra_joints[t];
    const Joint &jt = c.joints[joint];
    const PairBody a = load_pair_body(c, jt.body_a), b = load_pair_body(c, jt.body_b);
    const double hh = h * h;
    const double compliance = 1e-6 / hh;
    const Vec3 anchor_a{jt.anchor_a[0], jt.anchor_a[1], jt.anchor_a[2]}, anchor_b{jt.anchor_b[0], jt.anchor_b[1], jt.anchor_b[2]};
    const Vec3 axis_a{jt.axis_a[0], jt.axis_a[1], jt.axis_a[2]};
    const Vec3 p_a = Frame{frame_origin(a.pos, a.rot, a.com), a.rot} * anchor_a;
    const Vec3 p_b = Frame{frame_origin(b.pos, b.rot, b.com), b.rot} * anchor_b;
    const Vec3 d = p_b - p_a;
    const Vec3 a_w = a.rot * axis_a;
    const double s = dot(d, a_w);
    ExtraSum sum_a, sum_b;

    if (jt.kind == XPBD_JOINT_SLIDER) { // 1. the anchor of b is held to the axis of a
        const Vec3 r = d - a_w * s;
        const double len = length(r);
        if (len != 0.0) {
            const Vec3 n = r * (1.0 / len);
            const double w = generalized_inverse_mass(a, p_a, n) + generalized_inverse_mass(b, p_b, n);
            extra_linear_entry(a, b, p_a, p_b, n, len / (w + compliance), sum_a, sum_b);
        }
    }
    const uint32_t k_end = c.extra_off[t + 1];
    for (uint32_t k = c.extra_off[t]; k < k_end; ++k) { // 2. the SLIDE limit, 3. the drives in the caller's order
        const JointExtraItem &it = c.extra_items[k];
        const bool angular = it.kind == XPBD_DRIVE_ANGLE || it.kind == XPBD_DRIVE_ANGULAR_VELOCITY;
        double err, w;
        if (angular) {
            const Vec3 ref_a{it.ref_a[0], it.ref_a[1], it.ref_a[2]}, ref_b{it.ref_b[0], it.ref_b[1], it.ref_b[2]};
            const Vec3 r_a = a.rot * ref_a, r_b = b.rot * ref_b;
            const double phi = atan2(dot(cross(r_a, r_b), a_w), dot(r_a, r_b)); // as XPBD_LIMIT_HINGE
            if (it.kind == XPBD_DRIVE_ANGLE) {
                err = wrap_angle(phi - it.target);
            } else { // the same angle at the start of the substep
                const Vec3 a_w0 = a.past.rotation * axis_a;
                const Vec3 r_a0 = a.past.rotation * ref_a, r_b0 = b.past.rotation * ref_b;
                const double phi0 = atan2(dot(cross(r_a0, r_b0), a_w0), dot(r_a0, r_b0));
                err = wrap_angle(phi - phi0) - it.target * h;
            }
            const Vec3 n_a = conjugate(a.rot) * a_w, n_b = conjugate(b.rot) * a_w;
            w = dot(a.inv_inertia * n_a, n_a) + dot(b.inv_inertia * n_b, n_b);
        } else {
            if (it.kind == kExtraSlideLimit) {
                const double clamped = s < it.target ? it.target : (s > it.compliance ? it.compliance : s); // lower, upper
                err = s - clamped;
            } else if (it.kind == XPBD_DRIVE_POSITION) {
                err = s - it.target;
            } else { // XPBD_DRIVE_VELOCITY: the same offset at the start of the substep
                const Vec3 d0 = b.past * anchor_b - a.past * anchor_a;
                const double s0 = dot(d0, a.past.rotation * axis_a);
                err = (s - s0) - it.target * h;
            }
            w = generalized_inverse_mass(a, p_a, a_w) + generalized_inverse_mass(b, p_b, a_w);
        }
        if (err == 0.0)
            continue;
        double lambda;
        if (it.kind == kExtraSlideLimit) {
            lambda = err / (w + compliance);
        } else {
            lambda = err / (w + (1e-6 + it.compliance) / hh);
            const double cap = it.max_force * hh;
            lambda = lambda > cap ? cap : (lambda < -cap ? -cap : lambda);
        }
        if (angular)
            extra_angular_entry(a, b, a_w, lambda, sum_a, sum_b);
        else
            extra_linear_entry(a, b, p_a, p_b, a_w, lambda, sum_a, sum_b);
    }
    store_extra_sum(c.joint_extra + (size_t)c.extra_slots[2 * t + 0] * kJointExtraDoubles, sum_a);
    store_extra_sum(c.joint_extra + (size_t)c.extra_slots[2 * t + 1] * kJointExtraDoubles, sum_b);
}

// ---------------------------------------------------------------------------------------------------
// Per substep, per body: restitution, the velocity pass after derive (include/xpbd.h, "RESTITUTION").
// ---------------------------------------------------------------------------------------------------
// What the pass needs of a body: pose and velocities after derive, velocities at the start of the substep, mass properties.
struct VelBody {
    Vec3 pos;
    Quat rot;
    Vec3 vel, ang, vel0, ang0;
    double inv_mass;
    Mat3 inv_inertia;
    Vec3 com;
};

// post: the 13 dynamic fields after derive (SoA, as b.dyn); start: velocity and angular velocity at the start of the substep,
// [6][stride]
__device__ __forceinline__ VelBody load_vel_body(const double *__restrict__ post, const double *__restrict__ start, uint32_t st,
                                                 const ContactBuffers &c, uint32_t i)
{
    const BodyDynamic d = load_dynamic(post, st, i);
    const StatRecord s = load_stat_record(c.stat_rec, c.stat_index ? c.stat_index[i] : i);
    VelBody v;
    v.pos = d.pos, v.rot = d.rot, v.vel = d.vel, v.ang = d.ang;
    v.vel0 = load3(start, 0, st, i);
    v.ang0 = load3(start, 3, st, i);
    v.inv_mass = s.inv_mass;
    v.inv_inertia = s.inv_inertia;
    v.com = s.com;
    return v;
}

constexpr uint32_t kRestitutionSweeps = XPBD_RESTITUTION_SWEEPS; // passes over the points of one manifold

__device__ __forceinline__ double max_restitution(double a, double b) { return a < b ? b : a; }

// One lane per body.  Reads the post-derive state of every body from `post` and the start-of-substep velocities from `start`,
// writes the body's whole end-of-substep state to b.dyn, which no lane of this launch reads.
// TERRAIN: the ground part looks the terrain's plane up at every vertex of the mask again (the pose has moved since the
// integrate + ground stage): outside the field the vertex makes no entry, inside the plane's normal stands for (0, 0, 1).
template <bool TERRAIN>
__global__ void __launch_bounds__(kBlock) k_restitution(BodyArrays b, const double *__restrict__ post, const double *__restrict__ start,
                                                        ShapeTable shapes, ContactBuffers c, const uint32_t *__restrict__ ground_masks)
{
    extern __shared__ double lds[]; // shape vertex tables, as in k_integrate_ground
    uint32_t *lds_off = reinterpret_cast<uint32_t *>(lds + 3 * shapes.total_verts);
    for (uint32_t k = threadIdx.x; k < 3 * shapes.total_verts; k += blockDim.x)
        lds[k] = shapes.verts[k];
    for (uint32_t k = threadIdx.x; k <= shapes.n_shapes; k += blockDim.x)
        lds_off[k] = shapes.offsets[k];
    __syncthreads();

    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n)
        return;
    const uint32_t st = b.stride;
    VelBody self = load_vel_body(post, start, st, c, i);
    const double e_self = c.restitution[i], threshold = c.bounce_threshold;
    const Vec3 centre = self.pos + self.com;

    // pair contacts: Jacobi over the manifolds on the post-derive velocities, neighbour order
    Vec3 dv{0.0, 0.0, 0.0}, dw{0.0, 0.0, 0.0};
    uint32_t count = 0;
    const uint32_t k_end = c.nbr_off[i + 1];
    for (uint32_t k = c.nbr_off[i]; k < k_end; ++k) {
        const uint32_t pair = c.nbr_pair[k];
        const uint32_t code = c.pair_codes[pair];
        const uint32_t n_points = code & ((1u << kPairCodeFeatureShift) - 1u);
        if (!n_points)
            continue;
        const uint32_t j = c.nbr[k];
        const double e = max_restitution(e_self, c.restitution[j]); // (the larger of two values: the same from both sides)
        if (!(e > 0.0))
            continue;
        const VelBody other = load_vel_body(post, start, st, c, j);
        const Vec3 centre_other = other.pos + other.com;
        const ContactManifold *m = c.manifolds + pair;
        const uint32_t feature = code >> kPairCodeFeatureShift;
        // roles and points exactly as pair_solve_derive_body forms them
        const bool self_is_a = i < j;
        const bool ref_is_a = feature != 1u;
        const bool self_is_inc = self_is_a != ref_is_a;
        const bool face = feature != 2u;
        const Plane ref_plane{Vec3{m->plane[0], m->plane[1], m->plane[2]}, m->plane[3]};
        // Sequential impulses inside the manifold, on copies of the two bodies' post-derive velocities: every point keeps the
        // impulse it has applied so far (never negative), kRestitutionSweeps passes in point order.  Both bodies of the pair
        // run the same sequence on the same values (3-vectors selected by role, w_inc + w_ref commutes): the same bits.
        Vec3 v_s = self.vel, w_s = self.ang, v_o = other.vel, w_o = other.ang;
        double total[kMaxManifoldPoints];
#pragma unroll
        for (uint32_t pt = 0; pt < kMaxManifoldPoints; ++pt)
            total[pt] = 0.0;
        uint32_t applied = 0;
        for (uint32_t sweep = 0; sweep < kRestitutionSweeps; ++sweep) {
#pragma unroll
            for (uint32_t pt = 0; pt < kMaxManifoldPoints; ++pt) { // (unrolled: total[] stays in registers)
                if (pt >= n_points)
                    break;
                const Vec3 p_inc{m->point[pt][0], m->point[pt][1], m->point[pt][2]};
                Vec3 p_ref, n;
                if (face) {
                    const double depth = distance(ref_plane, p_inc);
                    p_ref = p_inc - depth * ref_plane.normal;
                    n = ref_plane.normal;
                } else {
                    p_ref = Vec3{m->point[1][0], m->point[1][1], m->point[1][2]};
                    const Vec3 d = p_ref - p_inc;
                    const double len = length(d);
                    if (len == 0.0)
                        continue;
                    n = d * (1.0 / len);
                }
                const Vec3 p_self = self_is_inc ? p_inc : p_ref, p_other = self_is_inc ? p_ref : p_inc;
                const Vec3 arm = p_self - centre, arm_other = p_other - centre_other;
                const Vec3 u_self = v_s + cross(w_s, arm), u_other = v_o + cross(w_o, arm_other);
                const Vec3 u0_self = self.vel0 + cross(self.ang0, arm), u0_other = other.vel0 + cross(other.ang0, arm_other);
                const double vn = dot(n, self_is_inc ? u_self - u_other : u_other - u_self);      // incident - reference
                const double vn0 = dot(n, self_is_inc ? u0_self - u0_other : u0_other - u0_self);
                // w = w_incident + w_reference; IEEE addition commutes
                const double w = generalized_inverse_mass(self, p_self, n) + generalized_inverse_mass(other, p_other, n);
                if (!(vn0 < -threshold && w > 0.0))
                    continue;
                double wanted = total[pt] + ((-e) * vn0 - vn) / w;
                if (!(wanted > 0.0))
                    wanted = 0.0;
                const double lambda = wanted - total[pt];
                if (lambda == 0.0)
                    continue;
                total[pt] = wanted;
                const Vec3 plus = lambda * n, minus = (-lambda) * n; // on the incident, on the reference body
                const Vec3 impulse = self_is_inc ? plus : minus, impulse_other = self_is_inc ? minus : plus;
                v_s = v_s + impulse * self.inv_mass;
                w_s = w_s + cross(self.inv_inertia * arm, impulse);
                v_o = v_o + impulse_other * other.inv_mass;
                w_o = w_o + cross(other.inv_inertia * arm_other, impulse_other);
                ++applied;
            }
        }
        if (applied) { // one Jacobi entry per manifold that bounced
            dv = dv + (v_s - self.vel);
            dw = dw + (w_s - self.ang);
            ++count;
        }
    }
    if (count) {
        const double cnt = (double)count;
        self.vel = self.vel + dv / cnt;
        self.ang = self.ang + dw / cnt;
    }

    // ground: the vertices of this substep's contact mask in vertex order, each applied at once
    const double e_ground = max_restitution(e_self, c.ground_restitution);
    const uint32_t mask = ground_masks[i];
    if (e_ground > 0.0 && mask) {
        const uint32_t sid = b.shape_id[i];
        const double *verts = lds + 3 * lds_off[sid];
        const Frame frame{frame_origin(self.pos, self.rot, self.com), self.rot};
        Vec3 n{0.0, 0.0, 1.0};
        const double target_scale = -e_ground;
        for (uint32_t todo = mask; todo != 0; todo &= todo - 1) {
            const uint32_t v = __ffs(todo) - 1;
            const Vec3 p = frame * Vec3{verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
            if (TERRAIN) {
                Plane plane;
                if (!terrain_plane(c.terrain, p, plane))
                    continue;
                n = plane.normal;
            }
            const Vec3 arm = p - centre;
            const double vn = dot(n, self.vel + cross(self.ang, arm));
            const double vn0 = dot(n, self.vel0 + cross(self.ang0, arm));
            const double w = generalized_inverse_mass(self, p, n);
            const double target = target_scale * vn0;
            if (!(vn0 < -threshold && vn < target && w > 0.0))
                continue;
            const double lambda = (target - vn) / w;
            const Vec3 impulse = lambda * n;
            self.vel = self.vel + impulse * self.inv_mass;
            self.ang = self.ang + cross(self.inv_inertia * arm, impulse);
        }
    }

    BodyDynamic d;
    d.pos = self.pos, d.rot = self.rot, d.vel = self.vel, d.ang = self.ang;
    store_dynamic(b.dyn, st, i, d);
}

// The pass has no subset form.  The bodies a BodySubset skips (the sleepers of a world with sleeping on) are put back
// afterwards from `post`, which holds their state as it was: one lane per body, 13 stores for a skipped one.
__global__ void __launch_bounds__(kBlock) k_restitution_put_back(BodyArrays b, const double *__restrict__ post, const uint8_t *__restrict__ skip)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n || !skip[i])
        return;
    for (uint32_t f = 0; f < kDynFields; ++f)
        b.dyn[(size_t)f * b.stride + i] = post[(size_t)f * b.stride + i];
}

// Halo exchange: one lane per (body, field); the buffer side is contiguous, the SoA side is a gather.
__global__ void k_export_dynamic(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, double *__restrict__ buf)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * kDynFields)
        return;
    const uint32_t k = t / kDynFields, f = t - k * kDynFields;
    buf[t] = b.dyn[(size_t)f * b.stride + indices[k]];
}

// (rows: optional; entry k of the list then comes from row rows[k] of buf instead of row k -- the gathered halo
// buffer of an all-gather can be imported as it is)
__global__ void k_import_dynamic(BodyArrays b, const uint32_t *__restrict__ indices, const uint32_t *__restrict__ rows, uint32_t n,
                                 const double *__restrict__ buf)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * kDynFields)
        return;
    const uint32_t k = t / kDynFields, f = t - k * kDynFields;
    b.dyn[(size_t)f * b.stride + indices[k]] = buf[(size_t)(rows ? rows[k] : k) * kDynFields + f];
}

// ---- body edits (include/xpbd.h, "Body EDITS") ----------------------------------------------------------------------------
// external_force / external_torque of the listed bodies: one lane per (entry, component), three force components and then
// three torque components; force / torque may be NULL (that field is left alone), indices NULL means body k.  An index
// outside the world is skipped.
__global__ void k_set_wrench(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, const double *__restrict__ force,
                             const double *__restrict__ torque)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 6u)
        return;
    const uint32_t k = t / 6u, f = t - k * 6u;
    const uint32_t i = indices ? indices[k] : k;
    if (i >= b.n)
        return;
    if (f < 3u) {
        if (force)
            b.stat[(size_t)(S_EXT_FORCE + f) * b.stride + i] = force[3 * (size_t)k + f];
    } else if (torque) {
        b.stat[(size_t)(S_EXT_TORQUE + (f - 3u)) * b.stride + i] = torque[3 * (size_t)k + (f - 3u)];
    }
}

// One xpbd_impulse (80 bytes = five 16-byte loads): {body | flags << 32, P.x} {P.y, P.z} {point.x, point.y}
// {point.z, L.x} {L.y, L.z}.
struct ImpulseEntry {
    uint32_t body, flags;
    Vec3 impulse, point, angular;
};

__device__ __forceinline__ ImpulseEntry load_impulse(const ulonglong2 *__restrict__ list, uint32_t k)
{
    const ulonglong2 *e = list + (size_t)k * 5;
    const ulonglong2 q0 = e[0], q1 = e[1], q2 = e[2], q3 = e[3], q4 = e[4];
    ImpulseEntry r;
    r.body = (uint32_t)q0.x;
    r.flags = (uint32_t)(q0.x >> 32);
    r.impulse = Vec3{__longlong_as_double((long long)q0.y), __longlong_as_double((long long)q1.x), __longlong_as_double((long long)q1.y)};
    r.point = Vec3{__longlong_as_double((long long)q2.x), __longlong_as_double((long long)q2.y), __longlong_as_double((long long)q3.x)};
    r.angular = Vec3{__longlong_as_double((long long)q3.y), __longlong_as_double((long long)q4.x), __longlong_as_double((long long)q4.y)};
    return r;
}

__device__ __forceinline__ uint32_t impulse_body(const ulonglong2 *__restrict__ list, uint32_t k)
{
    return reinterpret_cast<const uint32_t *>(list + (size_t)k * 5)[0];
}

// Impulses on the listed bodies, the entries of one body adjacent (a run) and applied in list order.  One lane per entry; the
// lane of a run's first entry does the whole run -- the body's mass properties, centre and velocities are loaded once, every
// entry is applied to the result of the one before with the restitution pass's impulse arithmetic, the velocities are stored
// once -- and the other lanes leave at once.  No two lanes write one body, so there are no atomics and the result does not
// depend on the launch shape.  A long run is serial in its lane by design (the order is the semantics); the lanes of a wave
// that have shorter runs wait for it.  A body outside the world is skipped.
__global__ void __launch_bounds__(kBlock) k_apply_impulses(BodyArrays b, const ulonglong2 *__restrict__ list, uint32_t n)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t i = impulse_body(list, k);
    if (k != 0 && impulse_body(list, k - 1) == i)
        return;
    if (i >= b.n)
        return;
    const uint32_t st = b.stride;
    const double inv_mass = b.stat[(size_t)S_INV_MASS * st + i];
    Mat3 inv_inertia;
    inv_inertia.cx = load3(b.stat, S_INV_INERTIA + 0, st, i);
    inv_inertia.cy = load3(b.stat, S_INV_INERTIA + 3, st, i);
    inv_inertia.cz = load3(b.stat, S_INV_INERTIA + 6, st, i);
    const Vec3 centre = load3(b.dyn, D_POS, st, i) + load3(b.stat, S_COM, st, i);
    Vec3 vel = load3(b.dyn, D_VEL, st, i), ang = load3(b.dyn, D_ANG, st, i);
    for (uint32_t j = k; j < n; ++j) {
        const ImpulseEntry e = load_impulse(list, j);
        if (e.body != i)
            break;
        vel = vel + e.impulse * inv_mass;
        if (!(e.flags & XPBD_IMPULSE_AT_CENTRE)) {
            const Vec3 arm = e.point - centre;
            ang = ang + cross(inv_inertia * arm, e.impulse);
        }
        ang = ang + inv_inertia * e.angular;
    }
    store3(b.dyn, D_VEL, st, i, vel);
    store3(b.dyn, D_ANG, st, i, ang);
}

// Halo validity (multi-GPU): positions of the listed bodies when the halos were chosen ...
__global__ void k_snapshot_positions(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, double *__restrict__ snapshot)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const Vec3 p = load3(b.dyn, D_POS, b.stride, indices[k]);
    snapshot[3 * (size_t)k + 0] = p.x, snapshot[3 * (size_t)k + 1] = p.y, snapshot[3 * (size_t)k + 2] = p.z;
}

// ... and the largest squared distance any of them has travelled since: *out = max(*out, max_k |pos_k - snapshot_k|^2).
// Non-negative doubles order like their bit patterns, so the maximum is an integer atomicMax (one per workgroup); a NaN
// position counts as +inf.
// (scale: optional per-entry factor on the squared distance, e.g. 1 / allowance^2: the result is then a ratio)
__global__ void __launch_bounds__(kBlock) k_max_displacement2(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n,
                                                              const double *__restrict__ snapshot, const double *__restrict__ scale,
                                                              double *__restrict__ out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    double d2 = 0.0;
    if (k < n) {
        const Vec3 p = load3(b.dyn, D_POS, b.stride, indices[k]);
        const Vec3 d = p - Vec3{snapshot[3 * (size_t)k + 0], snapshot[3 * (size_t)k + 1], snapshot[3 * (size_t)k + 2]};
        d2 = dot(d, d);
        if (scale)
            d2 *= scale[k];
        if (!(d2 <= DBL_MAX))
            d2 = __longlong_as_double(0x7FF0000000000000ll);
    }
    for (uint32_t off = 32; off; off >>= 1) {
        const double o = __shfl_xor(d2, off, 64);
        d2 = o > d2 ? o : d2;
    }
    __shared__ double part[kBlock / 64];
    if ((threadIdx.x & 63u) == 0)
        part[threadIdx.x >> 6] = d2;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kBlock / 64; ++w)
            d2 = part[w] > d2 ? part[w] : d2;
        if (d2 > 0.0)
            atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(d2));
    }
}

// ---- re-planning the multi-GPU world without a host round trip of the bodies (xpbd_multi.cpp) --------------------------------
// The grid cell of the bounding-sphere centre (position + center_of_mass, as the host planner adds them) of the listed
// bodies: the same floor(c / edge), clamp and packing as xpbd_halo_cell_key, so the same bits.  *bad = the smallest list
// index with a non-finite centre (UINT32_MAX: none).
constexpr long long kHaloCellBias = 1ll << 20, kHaloCellLimit = kHaloCellBias - 4;

__device__ __forceinline__ long long halo_clamp_cell(double q)
{
    const double lim = (double)kHaloCellLimit;
    if (!(q >= -lim)) // NaN or far negative
        return -kHaloCellLimit;
    return q > lim ? kHaloCellLimit : (long long)q;
}

__global__ void k_cell_keys(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, double edge, long long *__restrict__ keys,
                            uint32_t *__restrict__ bad)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t i = indices ? indices[k] : k;
    const Vec3 p = load3(b.dyn, D_POS, b.stride, i), com = load3(b.stat, S_COM, b.stride, i);
    const double c[3] = {p.x + com.x, p.y + com.y, p.z + com.z};
    long long cell[3];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        finite = finite && fabs(c[a]) <= DBL_MAX;
        cell[a] = halo_clamp_cell(floor(c[a] / edge));
    }
    if (!finite)
        atomicMin(bad, k);
    keys[k] = ((cell[0] + kHaloCellBias) << 42) | ((cell[1] + kHaloCellBias) << 21) | (cell[2] + kHaloCellBias);
}

__device__ __forceinline__ uint32_t aos_slot_of_field(uint32_t f) // xpbd_rigid double index of SoA field f (dyn first, then stat)
{
    if (f < kDynFields) // pos 31-33, rot 34-37, vel 22-24, ang 25-27
        return f < 7 ? 31 + f : (f < 10 ? 22 + (f - 7) : 25 + (f - 10));
    const uint32_t g = f - kDynFields; // 0..21 identical; com 28-30
    return g < 22 ? g : 28 + (g - 22);
}

// out[k] = {xpbd_rigid of body indices[k] (38 doubles), its shape id as a double}: the plan-time record of a body
__global__ void k_gather_records(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, double *__restrict__ out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr uint32_t kFields = kDynFields + kStatFields;
    if (t >= n * (kFields + 1))
        return;
    const uint32_t k = t / (kFields + 1), f = t - k * (kFields + 1), i = indices[k];
    double *rec = out + (size_t)k * (kFields + 1);
    if (f == kFields)
        rec[kFields] = (double)b.shape_id[i];
    else
        rec[aos_slot_of_field(f)] = f < kDynFields ? b.dyn[(size_t)f * b.stride + i] : b.stat[(size_t)(f - kDynFields) * b.stride + i];
}

// The bodies of a new local world in AoS: body s comes from slot src[s] of the old world's AoS copy (src[s] >= 0) or is
// incoming record -src[s] - 1 (39 doubles each: xpbd_rigid + shape id).
__global__ void k_repack_bodies(const double *__restrict__ old_aos, const uint32_t *__restrict__ old_shape, const int32_t *__restrict__ src,
                                uint32_t n_new, const double *__restrict__ incoming, double *__restrict__ new_aos,
                                uint32_t *__restrict__ new_shape)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr uint32_t kFields = kDynFields + kStatFields;
    if (t >= (size_t)n_new * kFields)
        return;
    const uint32_t s = (uint32_t)(t / kFields), f = (uint32_t)(t - (size_t)s * kFields);
    const int32_t from = src[s];
    if (from >= 0) {
        new_aos[t] = old_aos[(size_t)from * kFields + f];
        if (f == 0)
            new_shape[s] = old_shape[from];
    } else {
        const double *rec = incoming + (size_t)(-(from + 1)) * (kFields + 1);
        new_aos[t] = rec[f];
        if (f == 0)
            new_shape[s] = (uint32_t)rec[kFields];
    }
}

uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

} // namespace

// ---------------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------------
hipError_t launch_exclusive_scan(uint32_t *data, uint32_t n, uint32_t *scratch, hipStream_t stream)
{
    const uint32_t nb = (n + kBlock * 4 - 1) / (kBlock * 4);
    if (nb == 0) {
        return hipMemsetAsync(data, 0, sizeof(uint32_t), stream);
    }
    hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(kBlock), 0, stream, data, n, scratch);
    hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(kBlock), 0, stream, scratch, nb);
    hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(kBlock), 0, stream, data, n, scratch, nb);
    return hipGetLastError();
}

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

// Which form of the neighbour kernels a broadphase runs: bit 0 = group / mask test, bit 1 = jointed-pair test (only when
// there are joints).  A world without filters runs the plain form, the loads of which are those of a world before filters.
// Bit 2 = both-ends-inert test (only with sleeping on): the kernels that take the table.
static uint32_t filter_variant(const ContactBuffers &c, const InertBodies &inert)
{
    return (c.filter ? 1u : 0u) | (c.filter_jointed && c.joint_off ? 2u : 0u) | (inert.inert ? 4u : 0u);
}

hipError_t launch_neighbour_count(const BodyArrays &b, const ContactBuffers &c, hipStream_t stream, const InertBodies &inert)
{
    if (b.n) {
        const dim3 grid((b.n + kBodiesPerBlock - 1) / kBodiesPerBlock);
        switch (filter_variant(c, inert)) {
        case 0: hipLaunchKernelGGL((k_neighbour_count<false, false>), grid, dim3(kBlock), 0, stream, b, c); break;
        case 1: hipLaunchKernelGGL((k_neighbour_count<true, false>), grid, dim3(kBlock), 0, stream, b, c); break;
        case 2: hipLaunchKernelGGL((k_neighbour_count<false, true>), grid, dim3(kBlock), 0, stream, b, c); break;
        case 3: hipLaunchKernelGGL((k_neighbour_count<true, true>), grid, dim3(kBlock), 0, stream, b, c); break;
        case 4: hipLaunchKernelGGL((k_neighbour_count<false, false>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
        case 5: hipLaunchKernelGGL((k_neighbour_count<true, false>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
        case 6: hipLaunchKernelGGL((k_neighbour_count<false, true>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
        default: hipLaunchKernelGGL((k_neighbour_count<true, true>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
        }
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
    switch (filter_variant(c, inert)) {
    case 0: hipLaunchKernelGGL((k_neighbour_fill<false, false>), grid, dim3(kBlock), 0, stream, b, c); break;
    case 1: hipLaunchKernelGGL((k_neighbour_fill<true, false>), grid, dim3(kBlock), 0, stream, b, c); break;
    case 2: hipLaunchKernelGGL((k_neighbour_fill<false, true>), grid, dim3(kBlock), 0, stream, b, c); break;
    case 3: hipLaunchKernelGGL((k_neighbour_fill<true, true>), grid, dim3(kBlock), 0, stream, b, c); break;
    case 4: hipLaunchKernelGGL((k_neighbour_fill<false, false>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
    case 5: hipLaunchKernelGGL((k_neighbour_fill<true, false>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
    case 6: hipLaunchKernelGGL((k_neighbour_fill<false, true>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
    default: hipLaunchKernelGGL((k_neighbour_fill<true, true>), grid, dim3(kBlock), 0, stream, b, c, inert); break;
    }
    hipLaunchKernelGGL(k_neighbour_pair_index, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, c);
    return hipGetLastError();
}

hipError_t launch_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                   uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row, hipStream_t stream,
                                   const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    const size_t lds_bytes = (size_t)s.total_verts * 3 * sizeof(double) + (size_t)(s.n_shapes + 1) * sizeof(uint32_t);
    auto launch = [&](auto trace, auto materials) {
        if (c.terrain.planes)
            hipLaunchKernelGGL((k_integrate_ground<decltype(trace)::value, decltype(materials)::value, true>), dim3(blocks_for(items)),
                               dim3(kBlock), lds_bytes, stream, b, s, h, c, subset, last_mask, trace_masks, trace_row);
        else
            hipLaunchKernelGGL((k_integrate_ground<decltype(trace)::value, decltype(materials)::value>), dim3(blocks_for(items)), dim3(kBlock),
                               lds_bytes, stream, b, s, h, c, subset, last_mask, trace_masks, trace_row);
    };
    if (trace_masks && c.friction)
        launch(std::true_type{}, std::true_type{});
    else if (trace_masks)
        launch(std::true_type{}, std::false_type{});
    else if (c.friction)
        launch(std::false_type{}, std::true_type{});
    else
        launch(std::false_type{}, std::false_type{});
    return hipGetLastError();
}

hipError_t launch_terrain_planes(const double *heights, const Terrain &t, double *planes, hipStream_t stream)
{
    const uint32_t cells = (t.nx - 1) * (t.ny - 1);
    hipLaunchKernelGGL(k_terrain_planes, dim3(blocks_for(cells)), dim3(kBlock), 0, stream, heights, t, planes);
    return hipGetLastError();
}

hipError_t launch_sample_terrain(const Terrain &t, const double *xy, uint32_t n, double *height, double *normal_xyz, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sample_terrain, dim3(blocks_for(n)), dim3(kBlock), 0, stream, t, xy, n, height, normal_xyz);
    return hipGetLastError();
}

hipError_t launch_sat_contact_pairs(const BodyArrays &b, const PolytopeTables &t, const ContactBuffers &c,
                                    uint32_t n_pairs, SatScratch *list, hipStream_t stream, bool dense)
{
    return launch_sat_contacts(b, t, c.rec, c.pairs, n_pairs, c.manifolds, c.pair_codes, list, stream, dense);
}

hipError_t launch_pair_solve_derive(const BodyArrays &b, double *dyn_out, double h, const ContactBuffers &c,
                                    hipStream_t stream, const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    auto launch = [&](auto lanes, auto materials) {
        constexpr uint32_t G = decltype(lanes)::value;
        hipLaunchKernelGGL((k_pair_solve_derive<G, decltype(materials)::value>), dim3(blocks_for(items * G)), dim3(kBlock), 0, stream, b,
                           dyn_out, h, c, subset);
    };
    using Wide = std::integral_constant<uint32_t, kMaxManifoldPoints>;
    using One = std::integral_constant<uint32_t, 1>;
    const bool small = b.n <= kSmallWorld;
    if (small && c.friction)
        launch(Wide{}, std::true_type{});
    else if (small)
        launch(Wide{}, std::false_type{});
    else if (c.friction)
        launch(One{}, std::true_type{});
    else
        launch(One{}, std::false_type{});
    return hipGetLastError();
}

hipError_t launch_joint_extras(double h, const ContactBuffers &c, hipStream_t stream)
{
    if (!c.joint_extra || c.n_extra_joints == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_joint_extras, dim3(blocks_for(c.n_extra_joints)), dim3(kBlock), 0, stream, h, c);
    return hipGetLastError();
}

hipError_t launch_restitution(const BodyArrays &b, const double *post, const double *start, const ShapeTable &s, const ContactBuffers &c,
                              const uint32_t *ground_masks, hipStream_t stream, const BodySubset &subset)
{
    if (b.n == 0)
        return hipSuccess;
    if (!c.restitution || post == b.dyn || start == b.dyn || subset.list)
        return hipErrorInvalidValue; // (the kernel writes b.dyn while other lanes read `post` and `start`; it has no list form)
    const size_t lds_bytes = (size_t)s.total_verts * 3 * sizeof(double) + (size_t)(s.n_shapes + 1) * sizeof(uint32_t);
    if (c.terrain.planes)
        hipLaunchKernelGGL(k_restitution<true>, dim3(blocks_for(b.n)), dim3(kBlock), lds_bytes, stream, b, post, start, s, c, ground_masks);
    else
        hipLaunchKernelGGL(k_restitution<false>, dim3(blocks_for(b.n)), dim3(kBlock), lds_bytes, stream, b, post, start, s, c, ground_masks);
    if (subset.skip)
        hipLaunchKernelGGL(k_restitution_put_back, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, post, subset.skip);
    return hipGetLastError();
}

hipError_t launch_pair_solve_integrate_ground(const BodyArrays &b, const ShapeTable &s, double h, const ContactBuffers &c,
                                              double *next_rec, uint32_t *last_mask, uint32_t *trace_masks, uint32_t trace_row,
                                              hipStream_t stream, const BodySubset &subset)
{
    const uint32_t items = subset.list ? subset.count : b.n;
    if (items == 0)
        return hipSuccess;
    const size_t lds_bytes = (size_t)s.total_verts * 3 * sizeof(double) + (size_t)(s.n_shapes + 1) * sizeof(uint32_t);
    auto launch_form = [&](auto trace, auto lanes, auto materials) {
        constexpr uint32_t G = decltype(lanes)::value;
        hipLaunchKernelGGL((k_pair_solve_integrate_ground<decltype(trace)::value, G, decltype(materials)::value>), dim3(blocks_for(items * G)),
                           dim3(kBlock), lds_bytes, stream, b, s, h, c, subset, next_rec, last_mask, trace_masks, trace_row);
    };
    auto launch = [&](auto trace, auto lanes) { // contact materials: uniform over the launch, see pair_solve_derive_body
        if (c.friction)
            launch_form(trace, lanes, std::true_type{});
        else
            launch_form(trace, lanes, std::false_type{});
    };
    using Wide = std::integral_constant<uint32_t, kMaxManifoldPoints>;
    using One = std::integral_constant<uint32_t, 1>;
    const bool small = b.n <= kSmallWorld;
    if (trace_masks && small)
        launch(std::true_type{}, Wide{});
    else if (trace_masks)
        launch(std::true_type{}, One{});
    else if (small)
        launch(std::false_type{}, Wide{});
    else
        launch(std::false_type{}, One{});
    return hipGetLastError();
}

hipError_t launch_body_frames_aos(const BodyArrays &b, double *frames, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_body_frames_aos, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, frames);
    return hipGetLastError();
}

hipError_t launch_export_dynamic(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *buf, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_export_dynamic, dim3(blocks_for(n * kDynFields)), dim3(kBlock), 0, stream, b, indices, n, buf);
    return hipGetLastError();
}

hipError_t launch_import_dynamic(const BodyArrays &b, const uint32_t *indices, const uint32_t *rows, uint32_t n, const double *buf,
                                 hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_import_dynamic, dim3(blocks_for(n * kDynFields)), dim3(kBlock), 0, stream, b, indices, rows, n, buf);
    return hipGetLastError();
}

hipError_t launch_set_wrench(const BodyArrays &b, const uint32_t *indices, uint32_t n, const double *force, const double *torque,
                             hipStream_t stream)
{
    if (n > kMaxEditEntries)
        return hipErrorInvalidValue;
    if (n && (force || torque))
        hipLaunchKernelGGL(k_set_wrench, dim3(blocks_for(n * 6u)), dim3(kBlock), 0, stream, b, indices, n, force, torque);
    return hipGetLastError();
}

hipError_t launch_apply_impulses(const BodyArrays &b, const xpbd_impulse *list, uint32_t n, hipStream_t stream)
{
    static_assert(sizeof(xpbd_impulse) == 80 && sizeof(ulonglong2) == 16, "an xpbd_impulse is five 16-byte loads");
    if (n > kMaxEditEntries || (reinterpret_cast<uintptr_t>(list) & 15u))
        return hipErrorInvalidValue;
    if (n)
        hipLaunchKernelGGL(k_apply_impulses, dim3(blocks_for(n)), dim3(kBlock), 0, stream, b, reinterpret_cast<const ulonglong2 *>(list), n);
    return hipGetLastError();
}

hipError_t launch_snapshot_positions(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *snapshot, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_snapshot_positions, dim3(blocks_for(n)), dim3(kBlock), 0, stream, b, indices, n, snapshot);
    return hipGetLastError();
}

hipError_t launch_max_displacement2(const BodyArrays &b, const uint32_t *indices, uint32_t n, const double *snapshot, const double *scale,
                                    double *out, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_max_displacement2, dim3(blocks_for(n)), dim3(kBlock), 0, stream, b, indices, n, snapshot, scale, out);
    return hipGetLastError();
}

hipError_t launch_cell_keys(const BodyArrays &b, const uint32_t *indices, uint32_t n, double edge, int64_t *keys, uint32_t *bad, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_cell_keys, dim3(blocks_for(n)), dim3(kBlock), 0, stream, b, indices, n, edge, reinterpret_cast<long long *>(keys), bad);
    return hipGetLastError();
}

hipError_t launch_gather_records(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *out, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_gather_records, dim3(blocks_for(n * (kDynFields + kStatFields + 1))), dim3(kBlock), 0, stream, b, indices, n, out);
    return hipGetLastError();
}

hipError_t launch_repack_bodies(const double *old_aos, const uint32_t *old_shape, const int32_t *src, uint32_t n_new, const double *incoming,
                                double *new_aos, uint32_t *new_shape, hipStream_t stream)
{
    if (n_new) {
        const size_t threads = (size_t)n_new * (kDynFields + kStatFields);
        hipLaunchKernelGGL(k_repack_bodies, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, old_aos, old_shape, src, n_new,
                           incoming, new_aos, new_shape);
    }
    return hipGetLastError();
}

hipError_t launch_body_frames(const BodyArrays &b, double *rec, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_body_frames, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, rec);
    return hipGetLastError();
}

hipError_t launch_stat_records(const BodyArrays &b, double *stat_rec, hipStream_t stream)
{
    if (b.n)
        hipLaunchKernelGGL(k_stat_records, dim3(blocks_for(b.n)), dim3(kBlock), 0, stream, b, stat_rec);
    return hipGetLastError();
}

} // namespace xpbd
