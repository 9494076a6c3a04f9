// xpbd_body_ops.hip -- per-body utilities for gfx950 that are no contact code: halo export / import, body edits, halo validity
// and the re-plan kernels of the multi-GPU world.  Split from xpbd_contacts.hip; declarations: xpbd_body_ops.h.  Of
// xpbd_contacts_device.hpp it uses kBlock and blocks_for.
//
// Determinism: the kernels move bits, except k_apply_impulses, where ONE lane applies the entries of a body in list order.
// Atomics are used on integers only (atomicMax on the bit pattern of a non-negative double, atomicMin on a list index), and a
// maximum or minimum does not depend on the order it is formed in.
#include "xpbd_body_ops.h"
#include "xpbd_contacts_device.hpp"

namespace xpbd {
namespace {

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

} // namespace

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

} // namespace xpbd
