// xpbd_body_ops.h -- per-body utilities that are no contact code: launchers for xpbd_body_ops.hip.  Halo export / import, body
// edits, halo validity and the re-plan kernels of the multi-GPU world.  Used by the world's edits and halo entry points, which
// the multi-GPU frame, plan and edit code reach through the C ABI.
#pragma once

#include <cstdint>
#include <hip/hip_runtime_api.h>

#include "xpbd_kernels.h"

namespace xpbd {

// Halo exchange: gather / scatter the 13 dynamic fields of the listed bodies, body-major buffer.
hipError_t launch_export_dynamic(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *buf, hipStream_t stream);
hipError_t launch_import_dynamic(const BodyArrays &b, const uint32_t *indices, const uint32_t *rows, uint32_t n, const double *buf,
                                 hipStream_t stream); // rows: NULL = row k of buf for entry k

// Body edits (include/xpbd.h, "Body EDITS"), device arrays, stream-ordered.  external_force / external_torque of body
// indices[k] (NULL: body k) = force / torque[3k..3k+2] (NULL: that field is left alone);  the impulses of `list` (16-byte
// aligned; the entries of one body adjacent) on the velocities of their bodies, in list order.  An index outside the world is
// skipped.  More than kMaxEditEntries entries, or a misaligned list, is hipErrorInvalidValue.
constexpr uint32_t kMaxEditEntries = 1u << 29;
hipError_t launch_set_wrench(const BodyArrays &b, const uint32_t *indices, uint32_t n, const double *force, const double *torque,
                             hipStream_t stream);
hipError_t launch_apply_impulses(const BodyArrays &b, const xpbd_impulse *list, uint32_t n, hipStream_t stream);

// Halo validity: snapshot[3k..3k+2] = position of body indices[k]; *out = max(*out, max_k scale[k] * |position - snapshot|^2)
// (scale == NULL: 1).
hipError_t launch_snapshot_positions(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *snapshot, hipStream_t stream);
hipError_t launch_max_displacement2(const BodyArrays &b, const uint32_t *indices, uint32_t n, const double *snapshot, const double *scale,
                                    double *out, hipStream_t stream);

// Re-planning the multi-GPU world on the device.  keys[k] = grid cell (xpbd_halo_cell_key, same bits) of body indices[k]
// (indices == NULL: body k), *bad = min(*bad, first list index with a non-finite centre);  out[k] = the 38 doubles of
// xpbd_rigid of body indices[k] + its shape id as a double;  new world (AoS + shape ids) from src[s] >= 0: slot of the old
// world's AoS copy, < 0: incoming record -src[s] - 1 (39 doubles each).
hipError_t launch_cell_keys(const BodyArrays &b, const uint32_t *indices, uint32_t n, double edge, int64_t *keys, uint32_t *bad, hipStream_t stream);
hipError_t launch_gather_records(const BodyArrays &b, const uint32_t *indices, uint32_t n, double *out, hipStream_t stream);
hipError_t launch_repack_bodies(const double *old_aos, const uint32_t *old_shape, const int32_t *src, uint32_t n_new, const double *incoming,
                                double *new_aos, uint32_t *new_shape, hipStream_t stream);

} // namespace xpbd
