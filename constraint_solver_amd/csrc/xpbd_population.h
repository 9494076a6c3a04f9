// xpbd_population.h -- host-callable launchers for the gfx950 kernels in xpbd_population.hip: removing and appending resident
// bodies on the device (include/xpbd.h, "Body POPULATION").  Every write position comes from a scan: no atomics.
#pragma once

#include <cstdint>
#include <hip/hip_runtime_api.h>

#include "xpbd_kernels.h"

namespace xpbd {

// remove[indices[k]] = 1 for k < n_indices (an index >= n is skipped; the same index twice writes the same byte twice).
hipError_t launch_population_mark(const uint32_t *indices, uint32_t n_indices, uint8_t *remove, uint32_t n, hipStream_t stream);

// From the removal flags of n bodies (nonzero = remove): old_to_new[i] = number of survivors among the bodies 0..i-1, or
// 0xFFFFFFFF for a removed body; src[new] = old for every survivor (ascending); prefix[n] = the survivor count.
// prefix: [n + 1] scratch; scan_scratch: >= n / 1024 + 2 uint32 (launch_exclusive_scan).
hipError_t launch_population_map(const uint8_t *remove, uint32_t n, uint32_t *prefix, uint32_t *scan_scratch, uint32_t *old_to_new, uint32_t *src,
                                 hipStream_t stream);

// The surviving bodies, SoA -> SoA in one pass: field f of new body s = field f of old body src[s] for s < n_keep, all 38
// fields and the shape id (src == NULL: src[s] = s, nobody was removed), written into fresh arrays of stride fresh.stride.
// The slots fresh.n .. fresh.stride - 1 (the padding) are zeroed; the slots n_keep .. fresh.n - 1 belong to appended bodies
// and are left to launch_aos_to_soa.
hipError_t launch_population_gather_bodies(const BodyArrays &old, const BodyArrays &fresh, const uint32_t *src, uint32_t n_keep, hipStream_t stream);

// A per-body table: fresh[s] = old[src[s]] for s < n_keep, fresh[s] = fill for n_keep <= s < n_new.  T: uint2 (collision
// filters) or double (friction, restitution).
hipError_t launch_population_gather_filters(const uint2 *old, uint2 *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, uint2 fill,
                                            hipStream_t stream);
hipError_t launch_population_gather_doubles(const double *old, double *fresh, const uint32_t *src, uint32_t n_keep, uint32_t n_new, double fill,
                                            hipStream_t stream);

} // namespace xpbd
