// walk_kernels.hpp — launch interface of the walks' floor lookup on the GPU (walk_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "walk_core.h"

namespace dg {

// A scan workgroup covers WALK_SCAN_BLOCK = 1024 probes, a power of two: 256 lanes x 4 consecutive probes.  With at most
// WALK_MAX_PROBES = 2^26 probes there are at most 2^16 block maxima, which one workgroup scans in 256 rounds of 256.
static_assert((WALK_SCAN_BLOCK & (WALK_SCAN_BLOCK - 1u)) == 0u && WALK_SCAN_BLOCK % 256u == 0u, "a scan block is a power of two and whole lanes");

// On `stream`, in order: dg_walk_locate (one lane per probe: BSP descent, value and valid ? index : 0), dg_walk_block_max (reduce),
// dg_walk_scan_sums (exclusive max-scan of the block maxima, one workgroup), dg_walk_scan_apply (inclusive max-scan of every block on top
// of its carry) and dg_walk_gather (floors[e] = value[last[end_of_tic[e]]]).  No workgroup waits on another: the levels are launches.
// P.n_probes in [1, WALK_MAX_PROBES], P.n_blocks = ceil(n_probes / WALK_SCAN_BLOCK), P.first[0] != 0, every end_of_tic < n_probes.
hipError_t launch_walk_locate(const WalkParams &P, hipStream_t stream);

}  // namespace dg
