// xpbd_sensors.hip -- SENSOR bodies (EXTENSION) for gfx950.  Semantics: include/xpbd.h, "SENSOR bodies"; layout of the work:
// xpbd_sensors.h.
//
// Integers only.  k_sensor_mask_codes is one lane per pair: eight bytes of the pair list, two flag bytes, one code byte in, one
// out.  The solid keys and the sensor list are flag + launch_exclusive_scan + write, as the report compacts its keys.  The
// occupancy is one wave per sensor over its neighbour list, 64 entries at a time: a ballot of "this entry's pair touched" gives
// every kept entry its place in neighbour order.  No LDS of its own and no atomic anywhere, so no result depends on the schedule.
#include <hip/hip_runtime.h>

#include "xpbd_scan.h"
#include "xpbd_sensors.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;

uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

__global__ void __launch_bounds__(kBlock) k_sensor_mask_codes(const uint2 *__restrict__ pairs, const uint8_t *__restrict__ sensor,
                                                              const uint8_t *__restrict__ codes, uint8_t *__restrict__ solve_codes, uint32_t n_pairs)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs)
        return;
    const uint2 ab = pairs[p];
    solve_codes[p] = (sensor[ab.x] | sensor[ab.y]) ? (uint8_t)0 : codes[p];
}

__device__ __forceinline__ bool solid(const unsigned long long key, const uint8_t *__restrict__ sensor)
{
    return (sensor[(uint32_t)(key >> 32)] | sensor[(uint32_t)key]) == 0;
}

__global__ void __launch_bounds__(kBlock) k_sensor_solid_flag(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ key_count,
                                                              uint32_t key_lanes, const uint8_t *__restrict__ sensor, uint32_t *__restrict__ flag)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < key_lanes)
        flag[s] = (s < *key_count && solid(keys[s], sensor)) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_sensor_solid_write(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ key_count,
                                                               uint32_t key_lanes, const uint8_t *__restrict__ sensor, const uint32_t *__restrict__ flag,
                                                               unsigned long long *__restrict__ out)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= key_lanes || s >= *key_count)
        return;
    const unsigned long long key = keys[s];
    if (solid(key, sensor))
        out[flag[s]] = key; // flag[s] <= s < key_lanes
}

__global__ void __launch_bounds__(kBlock) k_sensor_not_inert(const uint8_t *__restrict__ sensor, uint8_t *__restrict__ inert, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && sensor[i])
        inert[i] = 0;
}

__global__ void __launch_bounds__(kBlock) k_sensor_flag(const uint8_t *__restrict__ sensor, uint32_t n, uint32_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n)
        flag[i] = sensor[i] ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_sensor_list(const uint8_t *__restrict__ sensor, uint32_t n, const uint32_t *__restrict__ flag,
                                                        uint32_t *__restrict__ list)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && sensor[i])
        list[flag[i]] = i;
}

__global__ void __launch_bounds__(kBlock) k_sensor_gather(const uint8_t *__restrict__ old, uint8_t *__restrict__ fresh, const uint32_t *__restrict__ src,
                                                          uint32_t n_keep, uint32_t n_new)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < n_new)
        fresh[s] = s < n_keep ? old[src ? src[s] : s] : (uint8_t)0;
}

// One wave per sensor.  FILL == false: sensors[k] and the number of kept neighbours into offsets[k]; FILL == true (offsets
// scanned): the kept neighbours into hits[offsets[k] ..), those below `cap`.
template <bool FILL>
__global__ void __launch_bounds__(kBlock) k_sensor_overlaps(SensorFrame f, uint32_t *__restrict__ sensors, uint32_t *__restrict__ offsets,
                                                            xpbd_sensor_hit *__restrict__ hits, uint32_t cap)
{
    static_assert(sizeof(xpbd_sensor_hit) == 8, "xpbd_sensor_hit is {body, pair}");
    const uint32_t k = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (k >= f.n_sensors) // (the same in every lane of a wave)
        return;
    const uint32_t i = f.list[k];
    const uint32_t lo = f.nbr_off[i], hi = f.nbr_off[i + 1];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t kept = 0;
    const uint32_t first = FILL ? offsets[k] : 0u;
    for (uint32_t base = lo; base < hi; base += kWave) {
        const uint32_t e = base + lane;
        uint32_t pair = 0;
        bool keep = false;
        if (e < hi) {
            pair = f.nbr_pair[e];
            keep = f.touch[pair] != 0u;
        }
        const unsigned long long votes = __ballot(keep);
        if (FILL && keep) {
            const uint32_t at = first + kept + (uint32_t)__popcll(votes & below);
            if (at < cap)
                hits[at] = xpbd_sensor_hit{f.nbr[e], f.record_of[pair]};
        }
        kept += (uint32_t)__popcll(votes);
        if (hi - base <= kWave) // (base + kWave may wrap only beyond 2^32 - 64 entries; stop on the last chunk all the same)
            break;
    }
    if (!FILL && lane == 0) {
        sensors[k] = i;
        offsets[k] = kept;
    }
}

} // namespace

hipError_t launch_sensor_mask_codes(const uint32_t *pairs, const uint8_t *sensor, const uint8_t *codes, uint8_t *solve_codes, uint32_t n_pairs,
                                    hipStream_t stream)
{
    if (n_pairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sensor_mask_codes, dim3(blocks_of(n_pairs)), dim3(kBlock), 0, stream, reinterpret_cast<const uint2 *>(pairs), sensor, codes,
                       solve_codes, n_pairs);
    return hipGetLastError();
}

hipError_t launch_sensor_solid_keys(const unsigned long long *keys, const uint32_t *key_count, uint32_t key_lanes, const uint8_t *sensor, uint32_t *flag,
                                    uint32_t *scratch, unsigned long long *out, hipStream_t stream)
{
    if (key_lanes)
        hipLaunchKernelGGL(k_sensor_solid_flag, dim3(blocks_of(key_lanes)), dim3(kBlock), 0, stream, keys, key_count, key_lanes, sensor, flag);
    if (hipError_t e = launch_exclusive_scan(flag, key_lanes, scratch, stream))
        return e;
    if (key_lanes)
        hipLaunchKernelGGL(k_sensor_solid_write, dim3(blocks_of(key_lanes)), dim3(kBlock), 0, stream, keys, key_count, key_lanes, sensor, flag, out);
    return hipGetLastError();
}

hipError_t launch_sensor_not_inert(const uint8_t *sensor, uint8_t *inert, uint32_t n, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sensor_not_inert, dim3(blocks_of(n)), dim3(kBlock), 0, stream, sensor, inert, n);
    return hipGetLastError();
}

hipError_t launch_sensor_list(const uint8_t *sensor, uint32_t n, uint32_t *flag, uint32_t *scratch, uint32_t *list, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_sensor_flag, dim3(blocks_of(n)), dim3(kBlock), 0, stream, sensor, n, flag);
    if (hipError_t e = launch_exclusive_scan(flag, n, scratch, stream))
        return e;
    if (n)
        hipLaunchKernelGGL(k_sensor_list, dim3(blocks_of(n)), dim3(kBlock), 0, stream, sensor, n, flag, list);
    return hipGetLastError();
}

hipError_t launch_sensor_gather(const uint8_t *old, uint8_t *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, hipStream_t stream)
{
    if (n_new == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_sensor_gather, dim3(blocks_of(n_new)), dim3(kBlock), 0, stream, old, fresh, src, n_keep, n_new);
    return hipGetLastError();
}

hipError_t launch_sensor_overlaps(const SensorFrame &f, uint32_t *sensors, uint32_t *offsets, xpbd_sensor_hit *hits, uint32_t cap, uint32_t *scratch,
                                  hipStream_t stream)
{
    const uint32_t per_block = kBlock / kWave, blocks = f.n_sensors / per_block + (f.n_sensors % per_block ? 1u : 0u);
    if (blocks)
        hipLaunchKernelGGL(k_sensor_overlaps<false>, dim3(blocks), dim3(kBlock), 0, stream, f, sensors, offsets, hits, cap);
    if (hipError_t e = launch_exclusive_scan(offsets, f.n_sensors, scratch, stream))
        return e;
    if (blocks && cap)
        hipLaunchKernelGGL(k_sensor_overlaps<true>, dim3(blocks), dim3(kBlock), 0, stream, f, sensors, offsets, hits, cap);
    return hipGetLastError();
}

} // namespace xpbd
