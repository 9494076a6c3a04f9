// xpbd_scan.h -- exclusive scan of uint32 on the device: launcher for xpbd_scan.hip.  Used by the broadphase, the contact
// reports, the islands, the body population, the query grid, the overlap queries and the world edits; it knows none of them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime_api.h>

namespace xpbd {

// Exclusive scan of data[0..n) in place; data[n] receives the total.  scratch: >= n/1024 + 2 uint32.
hipError_t launch_exclusive_scan(uint32_t *data, uint32_t n, uint32_t *scratch, hipStream_t stream);
// What the host callers reserve for `scratch` (bytes), with room to spare.
inline size_t scan_scratch_bytes(size_t n) { return (n / 1024 + 8) * 4; }

} // namespace xpbd
