// xpbd_report.hip -- contact REPORTS (EXTENSION) for gfx950: which pairs touched in a frame, their last manifolds, and the
// begin / end events between frames.  Semantics: include/xpbd.h, "Contact REPORTS"; layout of the work: xpbd_report.h.
//
// Determinism: every order is made by a scan (launch_exclusive_scan) over an order the pair list already has; no atomic
// decides a position.  The kernels only read what the pipeline wrote, so a report changes no bit of the simulation.
#include "xpbd_report.h"
#include "xpbd_scan.h"
#include "xpbd_device.hpp"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

uint32_t blocks_of(uint32_t n) { return (n + kBlock - 1) / kBlock; }

__global__ void __launch_bounds__(kBlock) k_report_touch(const uint8_t *__restrict__ codes, uint32_t *__restrict__ touch, uint32_t n_pairs)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n_pairs && (codes[p] & ((1u << kPairCodeFeatureShift) - 1u)) != 0u)
        touch[p] += 1u;
}

// Is pair p reported (touched in the frame, and in a shard its lower body is owned)?
__device__ __forceinline__ bool reported(const ReportFrame &f, uint32_t p)
{
    return f.touch[p] != 0u && (!f.owned || f.owned[f.pairs[2 * (size_t)p]] != 0u);
}

__device__ __forceinline__ uint32_t global_of(const ReportFrame &f, uint32_t slot) { return f.global_id ? f.global_id[slot] : slot; }

__global__ void __launch_bounds__(kBlock) k_report_flag(ReportFrame f, uint32_t *__restrict__ flag)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < f.n_pairs)
        flag[p] = reported(f, p) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_report_keys(ReportFrame f, const uint32_t *__restrict__ flag, unsigned long long *__restrict__ keys,
                                                        uint32_t *__restrict__ sel, uint32_t *__restrict__ npts)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= f.n_pairs || !reported(f, p))
        return;
    const uint32_t s = flag[p];
    keys[s] = ((unsigned long long)global_of(f, f.pairs[2 * (size_t)p]) << 32) | global_of(f, f.pairs[2 * (size_t)p + 1]);
    sel[s] = p;
    npts[s] = f.codes[p] & ((1u << kPairCodeFeatureShift) - 1u);
}

// One lane per touching pair: its record and points.  The points are read as the pair solve reads them
// (xpbd_contacts.hip, pair_solve_derive_body: point_term): a face contact's reference point is the stored incident point
// projected onto the stored plane with Plane::project's expression; the one-point contact stores point[0] on the incident
// body and point[1] on the reference body.
__global__ void __launch_bounds__(kBlock) k_report_records(ReportFrame f, const unsigned long long *__restrict__ keys,
                                                           const uint32_t *__restrict__ sel, const uint32_t *__restrict__ first_point,
                                                           uint32_t k, xpbd_pair_contact *__restrict__ out,
                                                           xpbd_contact_point *__restrict__ points)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= k)
        return;
    const uint32_t p = sel[s];
    const uint32_t code = f.codes[p];
    const uint32_t n = code & ((1u << kPairCodeFeatureShift) - 1u);
    const uint32_t feature = n ? code >> kPairCodeFeatureShift : 0u;
    const uint32_t first = first_point[s];
    Vec3 normal{0.0, 0.0, 0.0};
    double depth = 0.0;
    if (n) {
        const ContactManifold &m = f.manifolds[p];
        const bool face = feature != XPBD_FEATURE_EDGES;
        const Plane ref_plane{Vec3{m.plane[0], m.plane[1], m.plane[2]}, m.plane[3]};
        for (uint32_t q = 0; q < n; ++q) {
            const Vec3 p_inc{m.point[q][0], m.point[q][1], m.point[q][2]};
            Vec3 p_ref;
            if (face) {
                const double d = distance(ref_plane, p_inc);
                p_ref = p_inc - d * ref_plane.normal;
            } else {
                p_ref = Vec3{m.point[1][0], m.point[1][1], m.point[1][2]};
            }
            const double gap = length(p_ref - p_inc);
            depth = gap > depth ? gap : depth;
            if (points) {
                xpbd_contact_point &o = points[first + q];
                o.p_ref[0] = p_ref.x, o.p_ref[1] = p_ref.y, o.p_ref[2] = p_ref.z;
                o.p_inc[0] = p_inc.x, o.p_inc[1] = p_inc.y, o.p_inc[2] = p_inc.z;
            }
            if (!face) { // one point; the direction reference - incident
                const Vec3 u = p_ref - p_inc;
                if (gap != 0.0)
                    normal = u * (1.0 / gap);
                break;
            }
        }
        if (face)
            normal = feature == XPBD_FEATURE_FACE_B ? Vec3{-ref_plane.normal.x, -ref_plane.normal.y, -ref_plane.normal.z} : ref_plane.normal;
    }
    xpbd_pair_contact r;
    r.body_a = (uint32_t)(keys[s] >> 32);
    r.body_b = (uint32_t)keys[s];
    r.substeps = f.touch[p];
    r.n_points = n;
    r.feature = feature;
    r.first_point = first;
    r.reserved[0] = r.reserved[1] = 0u;
    r.normal[0] = normal.x, r.normal[1] = normal.y, r.normal[2] = normal.z;
    r.depth = depth;
    out[s] = r;
}

// Is `key` in the ascending list[0..n)?  (about 20 probes at a million keys)
__device__ __forceinline__ bool contains(const unsigned long long *__restrict__ list, uint32_t n, unsigned long long key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const unsigned long long v = list[mid];
        if (v == key)
            return true;
        if (v < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

__global__ void __launch_bounds__(kBlock) k_report_event_flags(const unsigned long long *__restrict__ cur, uint32_t n_cur,
                                                               const unsigned long long *__restrict__ prev, uint32_t n_prev,
                                                               uint32_t *__restrict__ flag)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < n_cur)
        flag[s] = contains(prev, n_prev, cur[s]) ? 0u : 1u;
    else if (s < n_cur + n_prev)
        flag[s] = contains(cur, n_cur, prev[s - n_cur]) ? 0u : 1u;
}

__global__ void __launch_bounds__(kBlock) k_report_event_write(const unsigned long long *__restrict__ cur, uint32_t n_cur,
                                                               const unsigned long long *__restrict__ prev, uint32_t n_prev,
                                                               const uint32_t *__restrict__ flag, xpbd_contact_event *__restrict__ out)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_cur + n_prev || flag[s + 1] == flag[s])
        return;
    const unsigned long long key = s < n_cur ? cur[s] : prev[s - n_cur];
    xpbd_contact_event &e = out[flag[s]];
    e.body_a = (uint32_t)(key >> 32);
    e.body_b = (uint32_t)key;
    e.kind = s < n_cur ? XPBD_CONTACT_BEGIN : XPBD_CONTACT_END;
}

} // namespace

hipError_t launch_report_touch(const uint8_t *codes, uint32_t *touch, uint32_t n_pairs, hipStream_t stream)
{
    if (n_pairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_report_touch, dim3(blocks_of(n_pairs)), dim3(kBlock), 0, stream, codes, touch, n_pairs);
    return hipGetLastError();
}

hipError_t launch_report_keys(const ReportFrame &f, uint32_t *flag, uint32_t *scratch, unsigned long long *keys, uint32_t *sel,
                              uint32_t *npts, hipStream_t stream)
{
    if (f.n_pairs)
        hipLaunchKernelGGL(k_report_flag, dim3(blocks_of(f.n_pairs)), dim3(kBlock), 0, stream, f, flag);
    if (hipError_t e = launch_exclusive_scan(flag, f.n_pairs, scratch, stream))
        return e;
    if (f.n_pairs)
        hipLaunchKernelGGL(k_report_keys, dim3(blocks_of(f.n_pairs)), dim3(kBlock), 0, stream, f, flag, keys, sel, npts);
    return hipGetLastError();
}

hipError_t launch_report_records(const ReportFrame &f, const unsigned long long *keys, const uint32_t *sel, const uint32_t *first_point,
                                 uint32_t k, xpbd_pair_contact *out, xpbd_contact_point *points, hipStream_t stream)
{
    if (k == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_report_records, dim3(blocks_of(k)), dim3(kBlock), 0, stream, f, keys, sel, first_point, k, out, points);
    return hipGetLastError();
}

hipError_t launch_report_event_flags(const unsigned long long *cur, uint32_t n_cur, const unsigned long long *prev, uint32_t n_prev,
                                     uint32_t *flag, uint32_t *scratch, hipStream_t stream)
{
    const uint32_t n = n_cur + n_prev;
    if (n)
        hipLaunchKernelGGL(k_report_event_flags, dim3(blocks_of(n)), dim3(kBlock), 0, stream, cur, n_cur, prev, n_prev, flag);
    if (hipError_t e = launch_exclusive_scan(flag, n, scratch, stream))
        return e;
    return hipGetLastError();
}

hipError_t launch_report_event_write(const unsigned long long *cur, uint32_t n_cur, const unsigned long long *prev, uint32_t n_prev,
                                     const uint32_t *flag, xpbd_contact_event *out, hipStream_t stream)
{
    const uint32_t n = n_cur + n_prev;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_report_event_write, dim3(blocks_of(n)), dim3(kBlock), 0, stream, cur, n_cur, prev, n_prev, flag, out);
    return hipGetLastError();
}

} // namespace xpbd
