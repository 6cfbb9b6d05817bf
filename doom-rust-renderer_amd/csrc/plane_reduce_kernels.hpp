// plane_reduce_kernels.hpp — launch interface of the reduced-size depth and label planes on the GPU (plane_reduce_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "plane_reduce_core.h"

namespace dg {

// A workgroup of dg_plane_nearest covers one band of fy source rows of one frame and a run of whole output pixels whose source
// distances, widened to 16-byte pieces of 8, fit PLANE_REDUCE_SPAN columns: 256 lanes x one piece.
constexpr uint32_t PLANE_REDUCE_LANES = 256;
constexpr uint32_t PLANE_REDUCE_SPAN = PLANE_REDUCE_LANES * 8u;
// Output pixels per workgroup under box width fx: fx columns each, and up to 7 columns in front of the first down to a 16-byte boundary.
constexpr uint32_t plane_reduce_px_per_wg(uint32_t fx) { return (PLANE_REDUCE_SPAN - 7u) / fx; }
static_assert(plane_reduce_px_per_wg(REDUCE_MAX_FACTOR) >= 1u && plane_reduce_px_per_wg(1u) + 7u <= PLANE_REDUCE_SPAN, "a workgroup's run fits its span");

// The planes of n frames, frame-major: sources of W x H, destinations of ceil(W / fx) x ceil(H / fy).
struct PlaneReduceSrc { const int16_t *distance; const uint8_t *kind; const uint16_t *id; const uint8_t *cls; };
struct PlaneReduceDst { int16_t *distance; uint8_t *kind; uint16_t *id; uint8_t *cls; };

// n_frames frames of the source planes reduced by d (plane_reduce_desc_ok) into the destinations that are not NULL, on `stream`:
// 1 <= W, H <= 16384, n_frames >= 0.  A source is read only when its destination is there, except src.distance, which DG_PLANE_NEAREST
// always reads (it must be there).  16-bit planes 2-byte aligned, otherwise any alignment: the 16-byte kernel runs when 2 W is a multiple
// of 16 and src.distance is 16-byte aligned, the any-width one otherwise.  start / stop: optional timing events attached to the first /
// last dispatch (kernels.hpp).
hipError_t launch_plane_reduce(const PlaneReduceSrc &src, int W, int H, int n_frames, const dg_plane_reduce_desc &d, const PlaneReduceDst &dst,
                               hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
