// xpbd_mass_edit.hip -- MASS properties of resident bodies (EXTENSION) for gfx950.  Semantics: include/xpbd.h, "MASS properties
// of resident bodies"; the list: xpbd_mass_edit.h; the value rules and the DIRECT inversion: xpbd_mass_row.hpp.
//
// k_set_mass is one lane per entry: 13 loads of the row, the rules, for DIRECT the determinant, three cross products and ten
// divisions, a binary search of the kinematic table (ascending by body; at most ceil(log2(n)) + 1 probes, the bound is a kernel
// argument), with XPBD_MASS_KEEP_FRAME a gather of the body's 13 dynamic doubles and its old centre of mass and a scatter of
// position and velocity, and a scatter of the 13 mass doubles into the SoA static fields.  No shared memory, no atomics: two
// entries that name one body are told apart by k_mass_claim, which runs first where that can happen -- every valid entry
// stores its list index into owner[body] (a plain 4-byte store: one of them stays), and k_set_mass applies an entry only if
// the word holds its index.  Every expression is the header's, operand for operand; the unit is built without contraction.
// k_get_mass is one lane per (entry, value).
#include <hip/hip_runtime.h>

#include "xpbd_body_ops.h"
#include "xpbd_device.hpp"
#include "xpbd_mass_edit.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// Does the table hold an entry for `body`?  The interval halves with every probe; `probes` bounds the walk all the same.
__device__ __forceinline__ bool kinematic_has(const KinematicTable &t, uint32_t probes, uint32_t body)
{
    uint32_t lo = 0, hi = t.n;
    for (uint32_t step = 0; step < probes && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const uint32_t at = t.entries[mid].body;
        if (at == body)
            return true;
        if (at < body)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return false;
}

// Entry k of the list: its body `i` and the 13 doubles `out` the body takes, or false (the entry is skipped).
__device__ __forceinline__ bool resolve_entry(const BodyArrays &b, const KinematicTable &t, uint32_t probes, const MassEditList &e, uint32_t k,
                                              uint32_t &i, double (&out)[kMassRowDoubles])
{
    i = e.indices ? e.indices[k] : k;
    if (i >= b.n)
        return false;
    double row[kMassRowDoubles];
#pragma unroll
    for (uint32_t c = 0; c < kMassRowDoubles; ++c)
        row[c] = e.rows[(size_t)k * kMassRowDoubles + c];
    if (resolve_mass_row(row, e.flags & kMassLayoutBits, out) != kMassRowOk)
        return false;
    return mass_row_fixed(out) || !kinematic_has(t, probes, i);
}

__global__ void __launch_bounds__(kBlock) k_mass_claim(BodyArrays b, KinematicTable t, uint32_t probes, MassEditList e)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= e.n)
        return;
    uint32_t i;
    double out[kMassRowDoubles];
    if (resolve_entry(b, t, probes, e, k, i, out))
        e.owner[i] = k;
}

__global__ void __launch_bounds__(kBlock) k_set_mass(BodyArrays b, KinematicTable t, uint32_t probes, MassEditList e)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= e.n)
        return;
    uint32_t i;
    double out[kMassRowDoubles];
    if (!resolve_entry(b, t, probes, e, k, i, out))
        return;
    if (e.owner && e.owner[i] != k)
        return;
    const uint32_t st = b.stride;
    if (e.flags & XPBD_MASS_KEEP_FRAME) {
        const Vec3 com = load3(b.stat, S_COM, st, i);
        const Vec3 pos = load3(b.dyn, D_POS, st, i), vel = load3(b.dyn, D_VEL, st, i), ang = load3(b.dyn, D_ANG, st, i);
        const Quat q = load_quat(b.dyn, D_ROT, st, i);
        const Vec3 d = Vec3{out[10], out[11], out[12]} - com;
        const Vec3 r = q * d;
        store3(b.dyn, D_POS, st, i, pos + (r - d));
        store3(b.dyn, D_VEL, st, i, vel + cross(ang, r));
    }
#pragma unroll
    for (uint32_t f = 0; f < kMassFixedDoubles; ++f)
        b.stat[(size_t)(S_INV_MASS + f) * st + i] = out[f];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c)
        b.stat[(size_t)(S_COM + c) * st + i] = out[kMassFixedDoubles + c];
}

__global__ void __launch_bounds__(kBlock) k_get_mass(BodyArrays b, const uint32_t *__restrict__ indices, uint32_t n, double *__restrict__ rows)
{
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)n * kMassRowDoubles)
        return;
    const uint32_t k = (uint32_t)(t / kMassRowDoubles), c = (uint32_t)(t - (size_t)k * kMassRowDoubles);
    const uint32_t i = indices ? indices[k] : k;
    const uint32_t field = c < kMassFixedDoubles ? S_INV_MASS + c : S_COM + (c - kMassFixedDoubles);
    rows[t] = i < b.n ? b.stat[(size_t)field * b.stride + i] : 0.0;
}

} // namespace

hipError_t launch_set_mass(const BodyArrays &b, const KinematicTable &kinematic, const MassEditList &list, hipStream_t stream)
{
    if (list.n > kMaxEditEntries || (reinterpret_cast<uintptr_t>(list.rows) & 7u) || !mass_flags_known(list.flags))
        return hipErrorInvalidValue;
    if (list.n == 0 || b.n == 0)
        return hipSuccess;
    if (!list.rows || (kinematic.n && !kinematic.entries))
        return hipErrorInvalidValue;
    uint32_t probes = 1; // ceil(log2(n)) + 1
    while (probes < 33u && (1ull << (probes - 1u)) < kinematic.n)
        ++probes;
    if (list.owner)
        hipLaunchKernelGGL(k_mass_claim, dim3(blocks_of(list.n)), dim3(kBlock), 0, stream, b, kinematic, probes, list);
    hipLaunchKernelGGL(k_set_mass, dim3(blocks_of(list.n)), dim3(kBlock), 0, stream, b, kinematic, probes, list);
    return hipGetLastError();
}

hipError_t launch_get_mass(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *rows, hipStream_t stream)
{
    if (n > kMaxEditEntries)
        return hipErrorInvalidValue;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_get_mass, dim3(blocks_of((uint64_t)n * kMassRowDoubles)), dim3(kBlock), 0, stream, b, indices, n, rows);
    return hipGetLastError();
}

} // namespace xpbd
