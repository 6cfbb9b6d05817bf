// depth_kernels.hpp — launch interface between the context (host) and depth_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "kernels.hpp"

namespace dg {

// dg_depth_tiles over every (frame, 64-column strip, band of rows) of the host lists P points at (frames, col_off, spans, walls, planes,
// the scene's opacity plane): dist[n_frames][H][W] and kind[n_frames][H][W], every pixel of every frame written.  P.rspans, P.fb and
// P.row_tab are not read.  start / stop: optional timing events attached to the dispatch (kernels.hpp).
hipError_t launch_depth(const RasterParams &P, int16_t *dist, uint8_t *kind, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
