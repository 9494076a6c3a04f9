// xpbd_kinematic.hip -- KINEMATIC bodies (EXTENSION) for gfx950.  Semantics: include/xpbd.h, "KINEMATIC bodies"; the table:
// xpbd_kinematic.h.
//
// k_kinematic_velocities is one lane per entry: the 64-byte entry, a gather of the body's position and rotation (7 doubles)
// from the SoA state and a scatter of its two velocities (6 doubles); with `moving` one byte more.  No shared memory, no
// atomics: the table is ascending by body, so no two lanes write the same body.  Every expression is the header's, operand for
// operand; the unit is built without contraction, as the stepper is.  k_kinematic_retarget is one lane per entry of a retarget
// list and writes seven doubles; k_kinematic_mass is one lane per entry and reads ten.
#include <hip/hip_runtime.h>

#include "xpbd_device.hpp"
#include "xpbd_kinematic.h"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

__global__ void __launch_bounds__(kBlock) k_kinematic_velocities(BodyArrays b, KinematicTable t, double h, uint32_t left, uint8_t *__restrict__ moving)
{
    static_assert(sizeof(xpbd_kinematic) == 64 && offsetof(xpbd_kinematic, linear) == 8, "xpbd_kinematic is {body, mode, linear[3], angular[4]}");
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= t.n)
        return;
    const xpbd_kinematic e = t.entries[k];
    const uint32_t i = e.body;
    if (i >= b.n)
        return; // (never: the setter refuses such an entry and a population change re-indexes the table)
    Vec3 vel, ang;
    if (e.mode == XPBD_KINEMATIC_POSE) {
        const Vec3 p = load3(b.dyn, D_POS, b.stride, i);
        const Quat q = load_quat(b.dyn, D_ROT, b.stride, i);
        const double r = (double)left;
        vel = (Vec3{e.linear[0], e.linear[1], e.linear[2]} - p) / (r * h);
        Quat dq = Quat{e.angular[0], e.angular[1], e.angular[2], e.angular[3]} * conjugate(q);
        if (dq.s < 0.0)
            dq = -dq;
        const Vec3 v = vec_of(dq);
        const double m = length(v);
        if (m == 0.0) {
            ang = Vec3{0.0, 0.0, 0.0};
        } else {
            const double half = atan2(m, dq.s);
            ang = v * ((2.0 / h) * tan(half / r) / m);
        }
    } else {
        vel = Vec3{e.linear[0], e.linear[1], e.linear[2]};
        ang = Vec3{e.angular[0], e.angular[1], e.angular[2]};
    }
    store3(b.dyn, D_VEL, b.stride, i, vel);
    store3(b.dyn, D_ANG, b.stride, i, ang);
    if (moving) // (a NaN component is nonzero: MOVING)
        moving[i] = (vel.x != 0.0 || vel.y != 0.0 || vel.z != 0.0 || ang.x != 0.0 || ang.y != 0.0 || ang.z != 0.0) ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_kinematic_retarget(KinematicTable t, const uint32_t *__restrict__ entries, const double *__restrict__ rows,
                                                               uint32_t n)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    uint32_t entry;
    if (!kinematic_entry_valid(t, entries, rows, k, entry))
        return;
    const double *row = rows + (size_t)k * kKinematicRowDoubles;
    double *dst = t.entries[entry].linear; // linear[3] and angular[4] are seven consecutive doubles
#pragma unroll
    for (uint32_t c = 0; c < kKinematicRowDoubles; ++c)
        dst[c] = row[c];
}

__global__ void __launch_bounds__(kBlock) k_kinematic_mass(BodyArrays b, KinematicTable t, double *__restrict__ out)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= t.n)
        return;
    const uint32_t i = t.entries[k].body;
#pragma unroll
    for (uint32_t f = 0; f < kKinematicMassDoubles; ++f)
        out[(size_t)k * kKinematicMassDoubles + f] = i < b.n ? b.stat[(size_t)(S_INV_MASS + f) * b.stride + i] : 0.0;
}

} // namespace

hipError_t launch_kinematic_velocities(const BodyArrays &b, const KinematicTable &t, double h, uint32_t left, uint8_t *moving, hipStream_t stream)
{
    if (t.n == 0 || b.n == 0)
        return hipSuccess;
    if (!t.entries || left == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kinematic_velocities, dim3(blocks_of(t.n)), dim3(kBlock), 0, stream, b, t, h, left, moving);
    return hipGetLastError();
}

hipError_t launch_kinematic_retarget(const KinematicTable &t, const uint32_t *entries, const double *rows, uint32_t n, hipStream_t stream)
{
    if (n == 0 || t.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_kinematic_retarget, dim3(blocks_of(n)), dim3(kBlock), 0, stream, t, entries, rows, n);
    return hipGetLastError();
}

hipError_t launch_kinematic_mass(const BodyArrays &b, const KinematicTable &t, double *out, hipStream_t stream)
{
    if (t.n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_kinematic_mass, dim3(blocks_of(t.n)), dim3(kBlock), 0, stream, b, t, out);
    return hipGetLastError();
}

} // namespace xpbd
