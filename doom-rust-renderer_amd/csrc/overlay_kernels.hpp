// overlay_kernels.hpp — launch interface of the screen pictures on the GPU (overlay_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "overlay_core.h"

namespace dg {

// The rectangle records rects[0, n_rects) of a plan (overlay_plan.hpp) and its items, both in device memory, drawn on the RGB24 frames
// of W x H at `frames` (device memory, any alignment), on `stream`: a workgroup per tile of a record, max_tiles the most tiles one record
// names.  palette: 256 x r | g << 8 | b << 16; idx / opq: the scene's texel planes, which hold every texel the items name.
// start / stop: optional timing events attached to the first / last dispatch (kernels.hpp).
hipError_t launch_overlay(uint8_t *frames, int W, int H, const OvlRect *rects, uint32_t n_rects, uint32_t max_tiles, const OvlItem *items, const uint32_t *palette,
                          const uint8_t *idx, const uint8_t *opq, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
