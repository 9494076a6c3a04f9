// xpbd_islands.hip -- contact ISLANDS (EXTENSION) for gfx950: connected groups of bodies and their rest state.  Semantics:
// include/xpbd.h, "Contact ISLANDS"; layout of the work: xpbd_islands.h.
//
// Grouping.  A lock-free union-find over parent[], which starts as the identity and only ever falls: parent[x] <= x at all
// times, and once parent[x] < x it stays below x.  One lane per edge finds the two roots with path halving and hooks the
// LARGER root under the smaller with a 32-bit compare-and-swap that only succeeds on a root.  No lane waits for another: a
// lost swap hands back the parent somebody else has just installed, and the lane goes on from there.  Every pass of a lane's
// loop strictly lowers one of its two indices or ends the lane, so a + b + 1 <= 2 n passes is a derived bound; the cap of
// 2 n + 2 is carried anyway and sets the give-up word.  A tree's root is below all its members, so the root of a finished
// component is its smallest member whichever lane hooked what: the result does not depend on the schedule.
//
// Numbering and records.  Root flags -> launch_exclusive_scan -> island ids in ascending order of the smallest member; no
// atomic decides a number.  The records are 32-bit integer adds and 64-bit integer maxima, which commute.  The settled pile
// is ONE island: every lane of every wave would hit the same record, so lanes that share a record are combined inside the
// wave first (ballot / popcount for the counts, a butterfly for the maxima) and one lane per distinct record issues the
// atomics.
//
// The kernels read the bodies, the masks, the report's keys and the joints, and write the unit's own scratch and the caller's
// outputs: a world's simulation is the same bits whether or not they ran.
#include <hip/hip_runtime.h>

#include "xpbd_islands.h"
#include "xpbd_scan.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kNone = XPBD_ISLAND_NONE;

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// parent[] while lanes race on it: relaxed, device-wide.
__device__ __forceinline__ uint32_t peek(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void poke(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kBlock) k_islands_init(IslandsWork w)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= w.n)
        return;
    bool fixed = true; // inverse_mass and all nine inverse_inertia entries == 0
#pragma unroll
    for (uint32_t f = 0; f < 10; ++f)
        fixed = fixed && w.stat[(size_t)(S_INV_MASS + f) * w.stride + i] == 0.0;
    w.parent[i] = i;
    w.fixed[i] = fixed ? 1 : 0;
}

// Edge t of the graph: the touching pairs first (lanes past the device's count carry none), then the joints.
struct Edge {
    uint32_t a, b;
    uint32_t joint; // 0: a touching pair, 1: a joint
    bool valid;
};

__device__ __forceinline__ Edge edge_of(const IslandsWork &w, uint64_t t)
{
    Edge e{0u, 0u, 0u, false};
    if (t < w.key_lanes) {
        if (t < *w.key_count) {
            const unsigned long long key = w.keys[t];
            e.a = (uint32_t)(key >> 32);
            e.b = (uint32_t)key;
            e.valid = true;
        }
    } else if (t - w.key_lanes < w.n_joints) {
        const Joint &j = w.joints[t - w.key_lanes];
        e.a = j.body_a;
        e.b = j.body_b;
        e.joint = 1u;
        e.valid = true;
    }
    e.valid = e.valid && e.a < w.n && e.b < w.n && e.a != e.b; // (always: both lists were checked when they were made)
    return e;
}

__global__ void __launch_bounds__(kBlock) k_islands_link(IslandsWork w)
{
    const Edge e = edge_of(w, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
    if (!e.valid || w.fixed[e.a] || w.fixed[e.b])
        return;
    uint32_t a = e.a, b = e.b;
    const uint64_t cap = 2ull * w.n + 2ull;
    for (uint64_t pass = 0;; ++pass) {
        if (pass >= cap) { // (never: each pass below lowers a or b, or returns)
            *w.status = 1u;
            return;
        }
        const uint32_t pa = peek(&w.parent[a]);
        if (pa != a) { // path halving: a's parent becomes its grandparent (an ancestor still, and parent[a] only falls)
            const uint32_t ga = peek(&w.parent[pa]);
            if (ga != pa)
                atomicMin(&w.parent[a], ga);
            a = ga;
            continue;
        }
        const uint32_t pb = peek(&w.parent[b]);
        if (pb != b) {
            const uint32_t gb = peek(&w.parent[pb]);
            if (gb != pb)
                atomicMin(&w.parent[b], gb);
            b = gb;
            continue;
        }
        if (a == b)
            return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t seen = atomicCAS(&w.parent[hi], hi, lo);
        if (seen == hi)
            return;
        // lost: hi is no root any more and `seen` < hi is its parent
        if (a == hi)
            a = seen;
        else
            b = seen;
    }
}

// parent[i] = root of i; flag[i] = i is the root of an island.  Lanes may read a parent another lane has already flattened:
// the old and the new value are both ancestors.
__global__ void __launch_bounds__(kBlock) k_islands_flatten(IslandsWork w)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= w.n)
        return;
    if (w.fixed[i]) {
        w.flag[i] = 0u;
        return;
    }
    uint32_t x = i;
    for (uint64_t step = 0;; ++step) {
        const uint32_t p = peek(&w.parent[x]);
        if (p == x)
            break;
        x = p;
        if (step > w.n) { // (never: x falls with every step)
            *w.status = 1u;
            break;
        }
    }
    if (x != i)
        poke(&w.parent[i], x);
    w.flag[i] = x == i ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_islands_zero(const uint32_t *__restrict__ total, xpbd_island *__restrict__ records, uint32_t cap)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= cap || s >= *total)
        return;
    xpbd_island r;
    r.first_body = r.n_bodies = r.n_pairs = r.n_joints = r.n_anchors = r.n_grounded = 0u;
    r.max_speed2 = r.max_angular_speed2 = 0.0;
    records[s] = r;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (uint32_t d = kWave / 2; d; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// v.x * v.x + v.y * v.y + v.z * v.z, left to right, as the bit pattern with the sign cleared (a NaN stays a NaN and beats all)
__device__ __forceinline__ unsigned long long speed2_bits(const double *dyn, uint32_t field, uint32_t stride, uint32_t i)
{
    const double x = dyn[(size_t)(field + 0) * stride + i], y = dyn[(size_t)(field + 1) * stride + i], z = dyn[(size_t)(field + 2) * stride + i];
    const double s = x * x + y * y + z * z;
    return (unsigned long long)__double_as_longlong(s) & 0x7FFFFFFFFFFFFFFFull;
}

// One lane per body: island_of, and the body's share of its island's record.
__global__ void __launch_bounds__(kBlock) k_islands_bodies(IslandsWork w, uint32_t *__restrict__ island_of, xpbd_island *__restrict__ records,
                                                           uint32_t cap)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & (kWave - 1);
    uint32_t id = kNone;
    bool root = false;
    if (i < w.n) {
        if (!w.fixed[i]) {
            const uint32_t r = w.parent[i];
            id = w.flag[r];
            root = r == i;
        }
        if (island_of)
            island_of[i] = id;
    }
    const bool mine = id < cap; // (kNone is not: cap <= 0xFFFFFFFF)
    unsigned long long v2 = 0, a2 = 0;
    bool grounded = false;
    if (mine) {
        v2 = speed2_bits(w.dyn, D_VEL, w.stride, i);
        a2 = speed2_bits(w.dyn, D_ANG, w.stride, i);
        grounded = w.last_mask[i] != 0u;
        if (root)
            records[id].first_body = i;
    }
    unsigned long long todo = __ballot(mine);
    while (todo) { // wave-uniform: one round per distinct island among the wave's lanes
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lid = __shfl(id, leader);
        const bool in = mine && id == lid;
        const unsigned long long group = __ballot(in);
        const uint32_t count = (uint32_t)__popcll(group), on_ground = (uint32_t)__popcll(__ballot(in && grounded));
        unsigned long long m_v = in ? v2 : 0ull, m_a = in ? a2 : 0ull;
        if (count > 1u) {
            m_v = wave_max(m_v);
            m_a = wave_max(m_a);
        }
        if (lane == leader) {
            xpbd_island &r = records[lid];
            atomicAdd(&r.n_bodies, count);
            if (on_ground)
                atomicAdd(&r.n_grounded, on_ground);
            atomicMax(reinterpret_cast<unsigned long long *>(&r.max_speed2), m_v);
            atomicMax(reinterpret_cast<unsigned long long *>(&r.max_angular_speed2), m_a);
        }
        todo &= ~group;
    }
}

// One lane per edge: n_pairs / n_joints of the island both ends are in, n_anchors of the island of the end that is not fixed.
__global__ void __launch_bounds__(kBlock) k_islands_edges(IslandsWork w, xpbd_island *__restrict__ records, uint32_t cap)
{
    const Edge e = edge_of(w, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint32_t id = kNone, which = 0u; // 0: n_pairs, 1: n_joints, 2: n_anchors
    if (e.valid) {
        const bool fa = w.fixed[e.a] != 0, fb = w.fixed[e.b] != 0;
        if (!(fa && fb)) {
            which = (fa || fb) ? 2u : e.joint;
            id = w.flag[w.parent[fa ? e.b : e.a]];
        }
    }
    const bool mine = id < cap;
    unsigned long long todo = __ballot(mine);
    while (todo) {
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lid = __shfl(id, leader), lwhich = __shfl(which, leader);
        const unsigned long long group = __ballot(mine && id == lid && which == lwhich);
        if (lane == leader) {
            xpbd_island &r = records[lid];
            atomicAdd(lwhich == 0u ? &r.n_pairs : (lwhich == 1u ? &r.n_joints : &r.n_anchors), (uint32_t)__popcll(group));
        }
        todo &= ~group;
    }
}

__global__ void k_islands_finish(const uint32_t *__restrict__ status, const uint32_t *__restrict__ k, uint32_t *__restrict__ total)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *total = *status ? kNone : *k;
}

} // namespace

hipError_t launch_islands(const IslandsWork &w, uint32_t *island_of, xpbd_island *records, uint32_t cap, uint32_t *total, hipStream_t stream)
{
    if (w.n == 0)
        return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(w.status, 0, sizeof(uint32_t), stream))
        return e;
    const uint64_t edges = (uint64_t)w.key_lanes + w.n_joints;
    if (edges > 0x7FFFFFFFull * kBlock)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_islands_init, dim3(blocks_of(w.n)), dim3(kBlock), 0, stream, w);
    if (edges)
        hipLaunchKernelGGL(k_islands_link, dim3(blocks_of(edges)), dim3(kBlock), 0, stream, w);
    hipLaunchKernelGGL(k_islands_flatten, dim3(blocks_of(w.n)), dim3(kBlock), 0, stream, w);
    if (hipError_t e = launch_exclusive_scan(w.flag, w.n, w.scan, stream))
        return e;
    if (cap) {
        const uint32_t most = cap < w.n ? cap : w.n; // K <= n
        hipLaunchKernelGGL(k_islands_zero, dim3(blocks_of(most)), dim3(kBlock), 0, stream, w.flag + w.n, records, most);
    }
    if (cap || island_of)
        hipLaunchKernelGGL(k_islands_bodies, dim3(blocks_of(w.n)), dim3(kBlock), 0, stream, w, island_of, records, cap);
    if (cap && edges)
        hipLaunchKernelGGL(k_islands_edges, dim3(blocks_of(edges)), dim3(kBlock), 0, stream, w, records, cap);
    hipLaunchKernelGGL(k_islands_finish, dim3(1), dim3(kWave), 0, stream, w.status, w.flag + w.n, total);
    return hipGetLastError();
}

} // namespace xpbd
