// xpbd_islands.h -- contact ISLANDS (EXTENSION): launcher for xpbd_islands.hip.  Semantics: include/xpbd.h, "Contact ISLANDS".
//
// One pass of connected components over what is already resident: the frame's touching pairs (the contact report's sorted
// keys, their count on the device), the joints, the mass properties and the last substep's ground-contact masks.  The
// grouping is a lock-free union-find under the invariant parent[x] <= x, so the root of a component is its smallest member
// whatever the schedule; the numbering is a scan over the root flags; the records are integer atomics (adds, and maxima over
// sign-cleared bit patterns), which commute.  Nothing here writes anything the stepper or the report reads.
#pragma once

#include "xpbd_contacts.h"

namespace xpbd {

struct IslandsWork {
    // inputs
    const double *dyn, *stat;   // the world's SoA bodies (xpbd_kernels.h)
    uint32_t stride, n;
    const uint32_t *last_mask;  // [n] ground contacts of the last substep
    const unsigned long long *keys; // the frame's touching pairs a << 32 | b, or NULL (no contact edges)
    const uint32_t *key_count;  // device: how many of them
    uint32_t key_lanes;         // host-side upper bound of *key_count (the frame's pair count): lanes launched
    const Joint *joints;        // or NULL (no joint edges)
    uint32_t n_joints;
    // scratch
    uint32_t *parent;           // [n]
    uint8_t *fixed;             // [n]
    uint32_t *flag;             // [n + 1] root flags, scanned in place: flag[root] = island id, flag[n] = K
    uint32_t *scan;             // scan_scratch_bytes(n)
    uint32_t *status;           // [1] give-up word: nonzero when a lane ran into its loop cap
};

// Enqueues the whole pass on `stream`.  island_of: [n] or NULL; records: the first min(K, cap) are written (cap == 0: none);
// *total = K, or XPBD_ISLAND_NONE when the give-up word is set.  All device pointers.
hipError_t launch_islands(const IslandsWork &w, uint32_t *island_of, xpbd_island *records, uint32_t cap, uint32_t *total, hipStream_t stream);

} // namespace xpbd
