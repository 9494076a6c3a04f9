// xpbd_query_overlap.hip -- scene queries (EXTENSION) for gfx950: overlap queries, convex volumes against the world's bodies.
// The decision of a pair (overlap_decide) and the candidate walk are in xpbd_query_device.hpp: the distance queries and the
// sweeps use them too.
#include "xpbd_query_units.hpp"

namespace xpbd {
namespace {

// ---- overlap queries: convex volumes against the bodies ------------------------------------------------------------------
// Semantics: include/xpbd.h, "Overlap queries".  One (query, body) pair is decided by three steps -- ignore_body and the group
// mask, the tight bounding spheres, the decision part of the SAT -- and both paths run the same routines for them, so the set
// of hits of a query does not depend on the path.  Neither does its order: the brute-force path visits the bodies in
// ascending index and reports them as it goes; the grid path reports them in cell order and k_overlap_sort brings every
// segment into ascending index (indices are distinct).  Every pass is run twice: once to count, once to fill, with an
// exclusive scan in between -- no list whose length the host would have to learn.
static_assert(sizeof(xpbd_overlap_query) == 72 && sizeof(xpbd_overlap_hit) == 16, "xpbd_overlap_query is 72 bytes, xpbd_overlap_hit 16");

// One lane per query: its bounding sphere, and whether it can report anything (finite frame, shape of the table).
__global__ void __launch_bounds__(kBlock) k_overlap_queries(const xpbd_overlap_query *__restrict__ queries, uint32_t n_queries, PolytopeTables t,
                                                            double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries)
        return;
    const xpbd_overlap_query &x = queries[q];
    const Frame f{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (x.shape < t.n_shapes) {
        const double *cc = t.centroids + 3 * (size_t)x.shape;
        c = f * Vec3{cc[0], cc[1], cc[2]};
        const bool finite = isfinite(f.position.x) && isfinite(f.position.y) && isfinite(f.position.z) && isfinite(f.rotation.s) &&
                            isfinite(f.rotation.x) && isfinite(f.rotation.y) && isfinite(f.rotation.z) && isfinite(c.x) && isfinite(c.y) &&
                            isfinite(c.z);
        const double rs = t.radii[x.shape];
        if (finite && rs >= 0.0)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

struct OverlapArgs : PassArgs {
    const xpbd_overlap_query *queries;
    uint32_t *offsets;          // count pass: offsets[q] = hits of q; fill pass: the scanned array
    xpbd_overlap_hit *hits;
    uint32_t cap;
};

// Count (FILL = false) or list (true) the hits of every query: one group of L lanes per query, 64 / L queries per wave.  The
// lanes of a group run steps 1 and 2 for one candidate each -- on the grid path each lane walks cells of its own out of the
// box of cells the query's sphere covers -- and the group then decides the survivors one after the other (step 3).
template <uint32_t L, uint32_t V, bool FILL>
__global__ void __launch_bounds__(64) k_overlap_pass(BodyArrays b, PolytopeTables t, OverlapArgs a)
{
    constexpr uint32_t PW = 64 / L;
    __shared__ OverlapLds<V> s_all[PW];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PW + group;
    if (q >= a.n)
        return;
    OverlapLds<V> &s = s_all[group];
    const double2 *qr = reinterpret_cast<const double2 *>(a.qrec + (size_t)q * kOverlapRecDoubles);
    const double2 q0 = qr[0], q1 = qr[1];
    const Vec3 cq{q0.x, q0.y, q1.x};
    const double rq = q1.y;
    // A segment the caller's buffer cuts short is listed in ascending order straight away (its first entries are what the
    // caller gets, and the sort needs whole segments); segments past the buffer are not listed at all.
    bool ordered = a.brute != 0;
    uint32_t base = 0, room = 0xFFFFFFFFu;
    if (FILL) {
        base = a.offsets[q];
        const uint32_t end = a.offsets[q + 1];
        if (end == base || base >= a.cap)
            return;
        ordered = ordered || end > a.cap;
        room = a.cap - base;
    }
    uint32_t count = 0;
    if (rq >= 0.0) {
        const xpbd_overlap_query &x = a.queries[q];
        const Frame fq{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}};
        const Frame fq_inv = inverse(fq);
        const uint32_t sq = x.shape, ignore = x.ignore_body, mask = x.mask;
        {
            const ShapeDesc dq = t.desc[sq];
            for (uint32_t vtx = lane; vtx < dq.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(dq.vert0 + vtx);
                st3(s.world[0], vtx, fq * Vec3{v[0], v[1], v[2]});
            }
        }
        // steps 1 and 2 of body i (one lane)
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            if (!admit_record(a, i, ignore, mask, centre, radius))
                return false;
            const Vec3 between = centre - cq;
            const double reach = rq + radius;
            return dot(between, between) < reach * reach;
        };
        // step 3 of the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                uint32_t feature = 0;
                double separation = 0.0;
                if (overlap_decide<L>(s, t, fq, fq_inv, sq, body_frame(b, i), b.shape_id[i], lane, feature, separation)) {
                    if (FILL && lane == 0 && count < room) {
                        xpbd_overlap_hit h;
                        h.body = a.gid ? a.gid[i] : i;
                        h.feature = feature;
                        h.separation = separation;
                        a.hits[base + count] = h;
                    }
                    ++count;
                }
            });
        };
        // the cells of the query on the grid, and whether walking them beats looking at every body
        QueryGrid g{};
        int32_t qlo[3] = {0, 0, 0};
        uint32_t qdim[3] = {1, 1, 1};
        bool walk = false;
        if (!ordered) {
            g = *a.grid;
            if (g.mode == kGrid) {
                const double c[3] = {cq.x, cq.y, cq.z};
                double cells = 1.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    qlo[ax] = clamp_axis(g, ax, floor((c[ax] - rq - g.pad) / g.edge));
                    const int32_t hi = clamp_axis(g, ax, floor((c[ax] + rq + g.pad) / g.edge));
                    qdim[ax] = (uint32_t)(hi - qlo[ax]) + 1u;
                    cells *= (double)qdim[ax];
                }
                walk = cells <= (double)g.mask + 1.0; // at most the cells a dense grid can have; beyond that, every body in turn
            }
        }
        if (walk)
            walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit, [](int, int32_t, int32_t) { return false; }, decide);
        else if (ordered || g.mode != kEmpty)
            // (its own loop, like the sweep pass's; see DESIGN, "One walk, measured")
            for (uint32_t i0 = 0; i0 < b.n && count < room; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
    }
    if (!FILL && lane == 0)
        a.offsets[q] = count;
}

// Every query's segment into ascending body order, one workgroup per query.  Indices are distinct: up to kOverlapSortStage
// entries are staged in LDS and each goes to the place its rank names; longer segments are sorted where they are, in global
// memory, by a bitonic network whose comparators all point upwards (entries past the end count as +inf and never move).
__global__ void __launch_bounds__(kBlock) k_overlap_sort(const uint32_t *__restrict__ offsets, xpbd_overlap_hit *__restrict__ hits, uint32_t cap)
{
    __shared__ xpbd_overlap_hit stage[kOverlapSortStage];
    const uint32_t b0 = offsets[blockIdx.x], b1 = offsets[blockIdx.x + 1];
    if (b1 > cap || b1 - b0 < 2)
        return; // (a segment the buffer cuts short was listed in order)
    const uint32_t len = b1 - b0;
    xpbd_overlap_hit *seg = hits + b0;
    if (len <= kOverlapSortStage) {
        for (uint32_t e = threadIdx.x; e < len; e += kBlock)
            stage[e] = seg[e];
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < len; e += kBlock) {
            const uint32_t id = stage[e].body;
            uint32_t rank = 0;
            for (uint32_t o = 0; o < len; ++o)
                rank += stage[o].body < id ? 1u : 0u;
            seg[rank] = stage[e];
        }
        return;
    }
    for (uint32_t k = 2; (k >> 1) < len; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < len; i += kBlock) {
                const uint32_t p = j == (k >> 1) ? i ^ (k - 1u) : i ^ j; // merge of two sorted runs: mirrored; then half-cleaners
                if (p > i && p < len) {
                    const xpbd_overlap_hit lo = seg[i], hi = seg[p];
                    if (lo.body > hi.body) {
                        seg[i] = hi;
                        seg[p] = lo;
                    }
                }
            }
            __syncthreads();
        }
}

} // namespace

hipError_t launch_overlap(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries_v,
                          uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, uint32_t *offsets, void *hits_v, uint32_t cap,
                          hipStream_t stream, const Terrain *terrain)
{
    if (n_queries == 0)
        return hipMemsetAsync(offsets, 0, sizeof(uint32_t), stream);
    brute = brute || b.n == 0;
    hipError_t e = hipSuccess;
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_overlap_queries, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, static_cast<const xpbd_overlap_query *>(queries_v),
                       n_queries, t, s.qrec);
    if (!brute && (e = launch_query_grid(b, s, stream)) != hipSuccess) // the grid of a ray cast, by the same passes
        return e;
    const OverlapArgs a{pass_args(s, global_id, filter, n_queries, masked, brute), static_cast<const xpbd_overlap_query *>(queries_v), offsets,
                        static_cast<xpbd_overlap_hit *>(hits_v), cap};
    auto pass = [&](auto fill) {
        with_group_shape(t, n_queries, [&](auto l, auto v, dim3 blocks) {
            hipLaunchKernelGGL((k_overlap_pass<decltype(l)::value, decltype(v)::value, decltype(fill)::value>), blocks, dim3(64), 0, stream, b, t, a);
        });
    };
    pass(std::false_type{});
    if (terrain && (e = launch_terrain_overlap(*terrain, t, queries_v, n_queries, false, s.qrec, offsets, hits_v, cap, stream)) != hipSuccess)
        return e;
    if ((e = launch_exclusive_scan(offsets, n_queries, s.scan_scratch, stream)) != hipSuccess)
        return e;
    if (cap) {
        pass(std::true_type{});
        // (before the sort, which takes whole segments: the terrain's index is the largest, so its entry stays the last)
        if (terrain && (e = launch_terrain_overlap(*terrain, t, queries_v, n_queries, true, s.qrec, offsets, hits_v, cap, stream)) != hipSuccess)
            return e;
        if (!brute)
            hipLaunchKernelGGL(k_overlap_sort, dim3(n_queries), dim3(kBlock), 0, stream, offsets, static_cast<xpbd_overlap_hit *>(hits_v), cap);
    }
    return hipGetLastError();
}

} // namespace xpbd
