// xpbd_terrain.hip -- heightfield terrain (include/xpbd.h, "TERRAIN") for gfx950: the plane table, once per
// xpbd_world_set_terrain, and the sampling call.  Split from xpbd_contacts.hip; declarations: xpbd_contacts.h.  The lookup the
// stepper and the sampling share (terrain_plane) is in xpbd_step.hpp; the terrain's scene queries: xpbd_terrain_query.hip.
//
// Determinism: one lane per cell or per point, no sums across lanes and no atomics.
#include "xpbd_contacts_device.hpp"

namespace xpbd {
namespace {

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

} // namespace

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

} // namespace xpbd
