// reduce_kernels.hpp — launch interface of the box downscale on the GPU (reduce_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "reduce_core.h"

namespace dg {

// A workgroup of dg_reduce covers one band of fy source rows of one frame and a run of whole output pixels whose source bytes,
// widened to 16-byte pieces, fit REDUCE_SPAN bytes: 256 lanes x one 16-byte piece.
constexpr uint32_t REDUCE_LANES = 256;
constexpr uint32_t REDUCE_SPAN = REDUCE_LANES * 16u;
// Output pixels per workgroup under box width fx: 3 fx bytes each, and up to 15 bytes in front of the first down to a 16-byte boundary.
constexpr uint32_t reduce_px_per_wg(uint32_t fx) { return (REDUCE_SPAN - 15u) / (3u * fx); }
static_assert(reduce_px_per_wg(REDUCE_MAX_FACTOR) >= 1u && 3u * reduce_px_per_wg(1u) + 15u <= REDUCE_SPAN, "a workgroup's run fits its span");

// n_frames RGB24 frames of W x H at src, reduced by d (reduce_desc_ok) into dst, on `stream`: 1 <= W, H <= 16384, n_frames >= 0.
// src and dst at any alignment: the 16-byte kernel runs when 3 W is a multiple of 16 and src is 16-byte aligned, the any-width one
// otherwise.  start / stop: optional timing events attached to the first / last dispatch (kernels.hpp).
hipError_t launch_reduce(const uint8_t *src, int W, int H, int n_frames, const dg_reduce_desc &d, uint8_t *dst, hipStream_t stream,
                         hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
