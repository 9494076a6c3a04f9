// xpbd_population.hip -- gfx950 kernels behind xpbd_world_remove_bodies / _add_bodies (include/xpbd.h, "Body POPULATION").
//
// Removal is a stream compaction: flags -> exclusive scan (launch_exclusive_scan, xpbd_scan.h) -> old_to_new and its
// inverse src[new] = old.  The scan makes every write position unique, so there are no atomics and the result does not
// depend on the schedule.  The gathers then read through src, which is ascending: lane l of a wave writes new body s0 + l of
// one field -- one 512-byte store per wave and field -- and reads old bodies that are at most as far apart as bodies were
// removed between them, so the loads of a wave fall into a few adjacent cache lines.  No arithmetic: the kernels move bits.
#include <hip/hip_runtime.h>

#include "xpbd_population.h"
#include "xpbd_scan.h"

namespace xpbd {
namespace {

constexpr uint32_t kPopBlock = 256;
constexpr uint32_t kGone = 0xFFFFFFFFu; // XPBD_NO_HIT

uint32_t pop_blocks(uint32_t n) { return (n + kPopBlock - 1) / kPopBlock; }

__global__ void __launch_bounds__(kPopBlock) k_population_mark(const uint32_t *__restrict__ indices, uint32_t n_indices, uint8_t *__restrict__ remove,
                                                               uint32_t n)
{
    const uint32_t k = blockIdx.x * kPopBlock + threadIdx.x;
    if (k >= n_indices)
        return;
    const uint32_t i = indices[k];
    if (i < n)
        remove[i] = 1;
}

__global__ void __launch_bounds__(kPopBlock) k_population_keep(const uint8_t *__restrict__ remove, uint32_t n, uint32_t *__restrict__ prefix)
{
    const uint32_t i = blockIdx.x * kPopBlock + threadIdx.x;
    if (i < n)
        prefix[i] = remove[i] ? 0u : 1u;
}

__global__ void __launch_bounds__(kPopBlock) k_population_map(const uint8_t *__restrict__ remove, uint32_t n, const uint32_t *__restrict__ prefix,
                                                              uint32_t *__restrict__ old_to_new, uint32_t *__restrict__ src)
{
    const uint32_t i = blockIdx.x * kPopBlock + threadIdx.x;
    if (i >= n)
        return;
    if (remove[i]) {
        old_to_new[i] = kGone;
        return;
    }
    const uint32_t s = prefix[i]; // survivors before i: < the survivor count <= n
    old_to_new[i] = s;
    src[s] = i;
}

// blockIdx.y == 0: the 13 dynamic fields and the shape id; 1: the 25 static fields.  One new body per lane.
template <uint32_t kFields>
__device__ __forceinline__ void gather_fields(const double *__restrict__ old, uint32_t old_stride, double *__restrict__ fresh, uint32_t stride,
                                              uint32_t s, uint32_t from, bool keep)
{
    double v[kFields];
#pragma unroll
    for (uint32_t f = 0; f < kFields; ++f)
        v[f] = keep ? old[(size_t)f * old_stride + from] : 0.0;
#pragma unroll
    for (uint32_t f = 0; f < kFields; ++f)
        fresh[(size_t)f * stride + s] = v[f];
}

__global__ void __launch_bounds__(kPopBlock) k_population_gather_bodies(BodyArrays old, BodyArrays fresh, const uint32_t *__restrict__ src,
                                                                        uint32_t n_keep)
{
    const uint32_t s = blockIdx.x * kPopBlock + threadIdx.x;
    if (s >= fresh.stride || (s >= n_keep && s < fresh.n)) // past the arrays / an appended body's slot
        return;
    uint32_t from = 0;
    bool keep = s < n_keep;
    if (keep) {
        from = src ? src[s] : s; // (NULL: nobody was removed)
        keep = from < old.n; // (always: src comes from k_population_map)
    }
    if (blockIdx.y == 0) {
        gather_fields<kDynFields>(old.dyn, old.stride, fresh.dyn, fresh.stride, s, from, keep);
        fresh.shape_id[s] = keep ? old.shape_id[from] : 0u;
    } else {
        gather_fields<kStatFields>(old.stat, old.stride, fresh.stat, fresh.stride, s, from, keep);
    }
}

template <class T>
__global__ void __launch_bounds__(kPopBlock) k_population_gather_table(const T *__restrict__ old, T *__restrict__ fresh, const uint32_t *__restrict__ src,
                                                                       uint32_t n_keep, uint32_t n_new, T fill)
{
    const uint32_t s = blockIdx.x * kPopBlock + threadIdx.x;
    if (s >= n_new)
        return;
    fresh[s] = s < n_keep ? old[src ? src[s] : s] : fill;
}

} // namespace

hipError_t launch_population_mark(const uint32_t *indices, uint32_t n_indices, uint8_t *remove, uint32_t n, hipStream_t stream)
{
    if (n_indices == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_population_mark, dim3(pop_blocks(n_indices)), dim3(kPopBlock), 0, stream, indices, n_indices, remove, n);
    return hipGetLastError();
}

hipError_t launch_population_map(const uint8_t *remove, uint32_t n, uint32_t *prefix, uint32_t *scan_scratch, uint32_t *old_to_new, uint32_t *src,
                                 hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_population_keep, dim3(pop_blocks(n)), dim3(kPopBlock), 0, stream, remove, n, prefix);
    if (hipError_t e = launch_exclusive_scan(prefix, n, scan_scratch, stream))
        return e;
    if (n)
        hipLaunchKernelGGL(k_population_map, dim3(pop_blocks(n)), dim3(kPopBlock), 0, stream, remove, n, prefix, old_to_new, src);
    return hipGetLastError();
}

hipError_t launch_population_gather_bodies(const BodyArrays &old, const BodyArrays &fresh, const uint32_t *src, uint32_t n_keep, hipStream_t stream)
{
    if (fresh.stride == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_population_gather_bodies, dim3(pop_blocks(fresh.stride), 2), dim3(kPopBlock), 0, stream, old, fresh, src, n_keep);
    return hipGetLastError();
}

hipError_t launch_population_gather_filters(const uint2 *old, uint2 *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, uint2 fill,
                                            hipStream_t stream)
{
    if (n_new == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_population_gather_table<uint2>, dim3(pop_blocks(n_new)), dim3(kPopBlock), 0, stream, old, fresh, src, n_keep, n_new, fill);
    return hipGetLastError();
}

hipError_t launch_population_gather_doubles(const double *old, double *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, double fill,
                                            hipStream_t stream)
{
    if (n_new == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_population_gather_table<double>, dim3(pop_blocks(n_new)), dim3(kPopBlock), 0, stream, old, fresh, src, n_keep, n_new, fill);
    return hipGetLastError();
}

} // namespace xpbd
