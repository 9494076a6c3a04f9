// xpbd_sleep.hip -- island SLEEPING (EXTENSION) for gfx950.  Semantics: include/xpbd.h, "SLEEPING"; layout of the work:
// xpbd_sleep.h.
//
// Every kernel is one lane per body (or per touching pair, or per list entry) with no shared memory.  What lanes share is
// written with integer atomics that commute -- or of a mark, add of a count, min of a counter -- so the state after a pass
// does not depend on the schedule.  Lanes of a wave that would hit the same word are combined first (ballot / popcount for
// the counts; a leader loop over the distinct islands for the minima, as k_islands_bodies does: the settled pile is ONE
// island).  A kernel that wakes or puts to sleep writes only its own body's words; the words other lanes read in the same
// launch (marks, island minima, parents) are written by an earlier launch.
#include <hip/hip_runtime.h>

#include "xpbd_device.hpp"
#include "xpbd_sleep.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kNoGroup = XPBD_SLEEP_GROUP_NONE;

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// inverse_mass and all nine inverse_inertia entries == 0 ("Contact ISLANDS")
__device__ __forceinline__ bool body_fixed(const double *__restrict__ stat, uint32_t stride, uint32_t i)
{
    bool fixed = true;
#pragma unroll
    for (uint32_t f = 0; f < 10; ++f)
        fixed = fixed && stat[(size_t)(S_INV_MASS + f) * stride + i] == 0.0;
    return fixed;
}

// One add per wave of the lanes for which `mine` holds (all lanes of the wave call it).
__device__ __forceinline__ void wave_count(uint32_t *counter, bool mine)
{
    const unsigned long long votes = __ballot(mine);
    if (votes && (threadIdx.x & (kWave - 1)) == (uint32_t)__ffsll((long long)votes) - 1u)
        atomicAdd(counter, (uint32_t)__popcll(votes));
}

// The group-wide wake.  stat != NULL (start of a frame): fixed[] is made here; else it is read.  `count`: the woken bodies
// are added to ctrl[SC_WOKEN].
__global__ void __launch_bounds__(kBlock) k_sleep_wake(SleepState s, const double *__restrict__ stat, uint32_t requests, bool count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool woke = false;
    if (i < s.n) {
        const uint32_t req = requests | s.ctrl[SC_REQUESTS];
        bool fixed;
        if (stat) {
            fixed = body_fixed(stat, s.stride, i);
            s.fixed[i] = fixed ? 1 : 0;
        } else {
            fixed = s.fixed[i] != 0;
        }
        bool asleep = s.asleep[i] != 0;
        if (asleep) {
            const uint32_t g = s.group[i];
            if ((req & kSleepWakeAll) || (g < s.n && s.mark[g] != 0u)) {
                s.asleep[i] = 0;
                s.rest_frames[i] = 0u;
                s.group[i] = kNoGroup;
                asleep = false;
                woke = true;
            }
        }
        if (req & kSleepZeroCounters)
            s.rest_frames[i] = 0u;
        s.inert[i] = (asleep || fixed) ? 1 : 0;
    }
    if (count)
        wave_count(&s.ctrl[SC_WOKEN], woke);
}

// One lane per touching pair of the frame: a sleeper that touches an awake body that is not fixed has its group marked.
__global__ void __launch_bounds__(kBlock) k_sleep_touch_mark(SleepState s, const unsigned long long *__restrict__ keys,
                                                             const uint32_t *__restrict__ key_count, uint32_t key_lanes)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= key_lanes || t >= *key_count)
        return;
    const unsigned long long key = keys[t];
    const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
    if (a >= s.n || b >= s.n)
        return; // (never: the keys come from the world's own pair list)
    const bool sa = s.asleep[a] != 0, sb = s.asleep[b] != 0;
    if (sa == sb)
        return;
    const uint32_t sleeper = sa ? a : b, other = sa ? b : a;
    if (s.fixed[other])
        return;
    const uint32_t g = s.group[sleeper];
    if (g < s.n)
        atomicOr(&s.mark[g], 1u);
}

// One lane per kinematic entry: a MOVING body is not inert (fixed, so never asleep).
__global__ void __launch_bounds__(kBlock) k_sleep_moving_inert(SleepState s, KinematicTable t)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= t.n)
        return;
    const uint32_t i = t.entries[k].body;
    if (i < s.n && s.moving[i])
        s.inert[i] = 0;
}

// One lane per pair of the frame's pair list, then one per joint: a sleeper that shares one with a MOVING body has its group
// marked (whether or not they touch: the rule is conservative).
__global__ void __launch_bounds__(kBlock) k_sleep_moving_mark(SleepState s, MovingBodies m)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t a, b;
    if (t < m.n_pairs) {
        a = m.pairs[2 * (size_t)t];
        b = m.pairs[2 * (size_t)t + 1];
    } else if (t - m.n_pairs < m.n_joints) {
        a = m.joints[t - m.n_pairs].body_a;
        b = m.joints[t - m.n_pairs].body_b;
    } else {
        return;
    }
    if (a >= s.n || b >= s.n)
        return; // (never: both come from the world's own tables)
    const bool ma = m.moving[a] != 0, mb = m.moving[b] != 0;
    if (ma == mb)
        return; // (two MOVING bodies are both fixed: neither sleeps)
    const uint32_t sleeper = ma ? b : a;
    if (!s.asleep[sleeper])
        return;
    const uint32_t g = s.group[sleeper];
    if (g < s.n)
        s.mark[g] = 1u; // (a plain store: every lane that writes the word writes this value)
}

// v.x * v.x + v.y * v.y + v.z * v.z, left to right (the unit is built without contraction)
__device__ __forceinline__ double speed2(const double *__restrict__ dyn, uint32_t field, uint32_t stride, uint32_t i)
{
    const double x = dyn[(size_t)(field + 0) * stride + i], y = dyn[(size_t)(field + 1) * stride + i], z = dyn[(size_t)(field + 2) * stride + i];
    return x * x + y * y + z * z;
}

// rest_frames of every awake body that is not fixed; and every island minimum starts at the top.
__global__ void __launch_bounds__(kBlock) k_sleep_count(SleepState s, const double *__restrict__ dyn, double linear2, double angular2)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= s.n)
        return;
    s.island_min[i] = 0xFFFFFFFFu;
    if (s.asleep[i] || s.fixed[i])
        return;
    // (a NaN fails both comparisons: not at rest)
    const bool at_rest = speed2(dyn, D_VEL, s.stride, i) <= linear2 && speed2(dyn, D_ANG, s.stride, i) <= angular2;
    const uint32_t before = s.rest_frames[i];
    s.rest_frames[i] = at_rest ? (before == 0xFFFFFFFFu ? before : before + 1u) : 0u;
}

// island_min[first body] = min over the island's members of rest_frames, a sleeper counting as 0.
__global__ void __launch_bounds__(kBlock) k_sleep_island_min(SleepState s, const uint32_t *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & (kWave - 1);
    uint32_t root = kNoGroup, value = 0u;
    bool mine = false;
    if (i < s.n && !s.fixed[i]) {
        root = parent[i];
        mine = root < s.n;
        value = s.asleep[i] ? 0u : s.rest_frames[i];
    }
    unsigned long long todo = __ballot(mine);
    while (todo) { // wave-uniform: one round per distinct island among the wave's lanes
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lroot = __shfl(root, leader);
        const bool in = mine && root == lroot;
        const unsigned long long group = __ballot(in);
        uint32_t m = in ? value : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t d = kWave / 2; d; d >>= 1) {
            const uint32_t o = __shfl_xor(m, d);
            m = o < m ? o : m;
        }
        if (lane == leader)
            atomicMin(&s.island_min[lroot], m);
        todo &= ~group;
    }
}

// An island all of whose members have rested long enough (none of them asleep: a sleeper made the minimum 0) goes to sleep.
__global__ void __launch_bounds__(kBlock) k_sleep_put(SleepState s, double *__restrict__ dyn, const uint32_t *__restrict__ parent,
                                                      const uint32_t *__restrict__ status, uint32_t frames_to_sleep)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool slept = false;
    if (i < s.n && !*status && !s.fixed[i] && !s.asleep[i]) {
        const uint32_t root = parent[i];
        if (root < s.n && s.island_min[root] >= frames_to_sleep) {
            s.asleep[i] = 1;
            s.group[i] = root;
#pragma unroll
            for (uint32_t f = 0; f < 6; ++f)
                dyn[(size_t)(D_VEL + f) * s.stride + i] = 0.0;
            slept = true;
        }
    }
    wave_count(&s.ctrl[SC_SLEPT], slept);
}

__global__ void __launch_bounds__(kBlock) k_sleep_records(SleepState s, BodyArrays b, double *__restrict__ rec_a, double *__restrict__ rec_b,
                                                          double *__restrict__ post, const uint32_t *__restrict__ last_mask,
                                                          uint32_t *__restrict__ trace, uint32_t trace_rows)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= s.n || !s.asleep[i])
        return;
    const Frame f = body_frame(b, i);
    const Vec3 pos = load3(b.dyn, D_POS, b.stride, i);
    const Quat rot = load_quat(b.dyn, D_ROT, b.stride, i);
    store_record(rec_a, i, f, f, pos, rot, pos);
    store_record(rec_b, i, f, f, pos, rot, pos);
    if (post)
        for (uint32_t k = 0; k < kDynFields; ++k)
            post[(size_t)k * b.stride + i] = b.dyn[(size_t)k * b.stride + i];
    if (trace) {
        const uint32_t mask = last_mask[i];
        for (uint32_t r = 0; r < trace_rows; ++r)
            trace[(size_t)r * b.stride + i] = mask;
    }
}

__global__ void __launch_bounds__(kBlock) k_sleep_request(SleepState s, const double *__restrict__ stat, const uint32_t *__restrict__ indices,
                                                          uint32_t every, uint32_t n)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t i = indices ? indices[(size_t)k * every] : k;
    if (i >= s.n)
        return;
    if (body_fixed(stat, s.stride, i)) {
        atomicOr(&s.ctrl[SC_REQUESTS], kSleepWakeAll); // an anchor may have moved
        return;
    }
    if (!s.asleep[i])
        return;
    const uint32_t g = s.group[i];
    if (g < s.n)
        atomicOr(&s.mark[g], 1u);
}

// One lane per entry of a retarget list (xpbd_world_set_drive_targets): the asleep ends of a valid entry's joint have their
// groups marked.  A fixed end is never asleep and its anchor did not move: it requests nothing.
__global__ void __launch_bounds__(kBlock) k_sleep_request_drives(SleepState s, DriveTable t, const Joint *__restrict__ joints, uint32_t n_joints,
                                                                 const uint32_t *__restrict__ drives, const double *__restrict__ targets, uint32_t n)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    uint32_t drive;
    if (!drive_entry_valid(t, drives, targets, k, drive))
        return;
    const uint32_t joint = t.items[t.drive_item[drive]].joint;
    if (joint >= n_joints)
        return; // (never: the items come from the world's own tables)
    const uint32_t ends[2] = {joints[joint].body_a, joints[joint].body_b};
#pragma unroll
    for (uint32_t e = 0; e < 2; ++e) {
        const uint32_t i = ends[e];
        if (i >= s.n || !s.asleep[i])
            continue;
        const uint32_t g = s.group[i];
        if (g < s.n)
            atomicOr(&s.mark[g], 1u);
    }
}

__global__ void __launch_bounds__(kBlock) k_sleep_tally(SleepState s)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool asleep = i < s.n && s.asleep[i] != 0;
    wave_count(&s.ctrl[SC_ASLEEP], asleep);
    wave_count(&s.ctrl[SC_GROUPS], asleep && s.group[i] == i);
}

} // namespace

hipError_t launch_sleep_frame_begin(const SleepState &s, const double *stat, uint32_t requests, hipStream_t stream)
{
    if (s.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_wake, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, stat, requests, false);
    if (hipError_t e = hipGetLastError())
        return e;
    if (hipError_t e = hipMemsetAsync(s.mark, 0, (size_t)s.n * 4, stream))
        return e;
    return hipMemsetAsync(s.ctrl + SC_REQUESTS, 0, 4, stream);
}

hipError_t launch_sleep_records(const SleepState &s, const BodyArrays &b, double *rec_a, double *rec_b, double *post, const uint32_t *last_mask,
                                uint32_t *trace, uint32_t trace_rows, hipStream_t stream)
{
    if (s.n == 0)
        return hipSuccess;
    if (!rec_a || !rec_b || s.n != b.n || s.stride != b.stride)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sleep_records, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, b, rec_a, rec_b, post, last_mask, trace, trace_rows);
    return hipGetLastError();
}

hipError_t launch_sleep_moving_inert(const SleepState &s, const KinematicTable &t, hipStream_t stream)
{
    if (s.n == 0 || t.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_moving_inert, dim3(blocks_of(t.n)), dim3(kBlock), 0, stream, s, t);
    return hipGetLastError();
}

hipError_t launch_sleep_wake_count(const SleepState &s, const double *dyn, const unsigned long long *keys, const uint32_t *key_count,
                                   uint32_t key_lanes, double linear2, double angular2, hipStream_t stream, const MovingBodies &moving)
{
    if (s.n == 0)
        return hipSuccess;
    if (hipError_t e = hipMemsetAsync(s.ctrl + SC_WOKEN, 0, 2 * 4, stream)) // SC_WOKEN, SC_SLEPT
        return e;
    const uint64_t moving_lanes = moving.moving ? (uint64_t)moving.n_pairs + moving.n_joints : 0u;
    if (moving_lanes)
        hipLaunchKernelGGL(k_sleep_moving_mark, dim3(blocks_of(moving_lanes)), dim3(kBlock), 0, stream, s, moving);
    if ((keys && key_lanes) || moving_lanes) {
        if (keys && key_lanes)
            hipLaunchKernelGGL(k_sleep_touch_mark, dim3(blocks_of(key_lanes)), dim3(kBlock), 0, stream, s, keys, key_count, key_lanes);
        hipLaunchKernelGGL(k_sleep_wake, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, (const double *)nullptr, 0u, true);
        if (hipError_t e = hipGetLastError())
            return e;
        if (hipError_t e = hipMemsetAsync(s.mark, 0, (size_t)s.n * 4, stream))
            return e;
    }
    hipLaunchKernelGGL(k_sleep_count, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, dyn, linear2, angular2);
    return hipGetLastError();
}

hipError_t launch_sleep_islands(const SleepState &s, double *dyn, const uint32_t *parent, const uint32_t *status, uint32_t frames_to_sleep,
                                hipStream_t stream)
{
    if (s.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_island_min, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, parent);
    hipLaunchKernelGGL(k_sleep_put, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s, dyn, parent, status, frames_to_sleep);
    return hipGetLastError();
}

hipError_t launch_sleep_request(const SleepState &s, const double *stat, const uint32_t *indices, uint32_t every, uint32_t n, hipStream_t stream)
{
    if (s.n == 0 || n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_request, dim3(blocks_of(n)), dim3(kBlock), 0, stream, s, stat, indices, every, n);
    return hipGetLastError();
}

hipError_t launch_sleep_request_drives(const SleepState &s, const DriveTable &t, const Joint *joints, uint32_t n_joints, const uint32_t *drives,
                                       const double *targets, uint32_t n, hipStream_t stream)
{
    if (s.n == 0 || n == 0 || t.n_drives == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_request_drives, dim3(blocks_of(n)), dim3(kBlock), 0, stream, s, t, joints, n_joints, drives, targets, n);
    return hipGetLastError();
}

hipError_t launch_sleep_tally(const SleepState &s, hipStream_t stream)
{
    if (hipError_t e = hipMemsetAsync(s.ctrl + SC_ASLEEP, 0, 2 * 4, stream)) // SC_ASLEEP, SC_GROUPS
        return e;
    if (s.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sleep_tally, dim3(blocks_of(s.n)), dim3(kBlock), 0, stream, s);
    return hipGetLastError();
}

} // namespace xpbd
