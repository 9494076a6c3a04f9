// xpbd_contacts_device.hpp -- contact pipeline (EXTENSION): what more than one of the units split from xpbd_contacts.hip uses.
// Not installed, and included only by those units.  Everything is in an anonymous namespace, as it was when they were one
// unit: every unit gets its own copy, the kernels that use a routine see it exactly as before, and no symbol crosses a unit.
//
// Who uses what:
//
//   routine                                   broadphase  contacts  restitution  terrain  body_ops
//   kBlock, blocks_for                             x          x          x          x        x
//   with_flag                                      x          x
//   generalized_inverse_mass                                  x          x
//   shape_lds_bytes, stage_shape_tables                       x          x
//
// xpbd_damping.hip (stage 7, not split from xpbd_contacts.hip) uses kBlock, blocks_for and generalized_inverse_mass.
// xpbd_scan.hip includes nothing of this: it serves units that are no part of the pipeline and keeps a kBlock of its own.
// What a single unit uses is in that unit: cell_hash ... for_each_neighbour (broadphase); min_mu, ground_mu, subset_body,
// store_row, load_row, PairBody ... block_add_stats, the joint helpers (contacts); VelBody, load_vel_body, max_restitution
// (restitution); ImpulseEntry, halo_clamp_cell, aos_slot_of_field (body_ops).
#pragma once

#include <cfloat>
#include <type_traits>

#include "xpbd_contacts.h"
#include "xpbd_step.hpp"

namespace xpbd {
namespace {

constexpr uint32_t kBlock = 256;

inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

// A run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{}).  The launchers choose the form of a
// kernel with it; which forms exist is decided by the calls, as it was by the ladders this replaces.
template <class F>
void with_flag(bool flag, F &&f)
{
    if (flag)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// Constraint::inverse_resitance for one body, src/constraint.rs:25-32
// (Body: PairBody -- the pose after the ground contacts -- or the velocity pass's VelBody, the pose after derive)
template <class Body>
__device__ __forceinline__ double generalized_inverse_mass(const Body &p, Vec3 point, Vec3 dir)
{
    const Vec3 angular_impulse = conjugate(p.rot) * cross(point - (p.pos + p.com), dir);
    return p.inv_mass + dot(p.inv_inertia * angular_impulse, angular_impulse);
}

// The shape vertex tables in LDS, as in k_step: 3 * total_verts doubles, then n_shapes + 1 offsets.  The launchers of the
// kernels that stage them pass shape_lds_bytes as the dynamic LDS size.
inline size_t shape_lds_bytes(const ShapeTable &s)
{
    return (size_t)s.total_verts * 3 * sizeof(double) + (size_t)(s.n_shapes + 1) * sizeof(uint32_t);
}

// Every thread of the workgroup calls this (it ends in a barrier): `lds` receives the vertices; returns the offsets behind them.
__device__ __forceinline__ uint32_t *stage_shape_tables(double *lds, const ShapeTable &shapes)
{
    uint32_t *lds_off = reinterpret_cast<uint32_t *>(lds + 3 * shapes.total_verts);
    for (uint32_t k = threadIdx.x; k < 3 * shapes.total_verts; k += blockDim.x)
        lds[k] = shapes.verts[k];
    for (uint32_t k = threadIdx.x; k <= shapes.n_shapes; k += blockDim.x)
        lds_off[k] = shapes.offsets[k];
    __syncthreads();
    return lds_off;
}

} // namespace
} // namespace xpbd
