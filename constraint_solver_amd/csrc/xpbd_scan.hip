// xpbd_scan.hip -- exclusive scan of uint32 for gfx950 (three small kernels; 1024 elements per block).  Split from
// xpbd_contacts.hip; its callers are listed in xpbd_scan.h.
//
// Determinism: integer sums only, every one formed in a fixed order (lane, wave, block); no atomics.  The result does not
// depend on the launch order.  This unit stands alone: it has its own kBlock (as xpbd_report.hip and xpbd_population.hip have
// theirs) and includes nothing of the contact pipeline.
#include <hip/hip_runtime.h>

#include "xpbd_scan.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

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

} // namespace

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

} // namespace xpbd
