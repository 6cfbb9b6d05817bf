// map_kernels.hpp — launch interface of the 2-D map view's kernels (map_kernels.hip).
//
// A map frame is a view-independent layer (every drawn linedef, built once per uploaded scene) plus the player arrow of that view.
//   layer     : launch_map_layer  — one lane per (line, clipped step): atomicMax(owner[pixel], line + 1), then owner -> RGB24
//   per frame : launch_map_frames — copy of the layer into every frame of the batch (non-temporal stores), then the arrow's steps
//   arrow     : launch_map_arrow  — the arrow's steps alone, on top of frames somebody else filled (explored_kernels.hip)
#pragma once
#include <hip/hip_runtime_api.h>

#include "map_core.h"

namespace dg {

// Renders lines segs[0 .. n) (clipped by map_seg_make; base[k] = sum of the counts before line k, base[n] = total) into layer
// (3*W*H bytes), later lines over earlier ones, black where no line is.  owner: W*H u32 scratch.  start / stop as in kernels.hpp.
hipError_t launch_map_layer(const MapSeg *segs, const uint32_t *base, uint32_t n, uint32_t total, uint32_t *owner, uint8_t *layer,
                            int W, int H, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// fb frame f = layer, then arrow[3f .. 3f + 3) drawn on top, for f in [0, n_frames).  start: on the copy, stop: on the arrow kernel.
hipError_t launch_map_frames(const uint8_t *layer, const MapSeg *arrow, int n_frames, uint8_t *fb, int W, int H, hipStream_t stream,
                             hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// arrow[3f .. 3f + 3) drawn into fb frame f, for f in [0, n_frames): dg_map_arrow over (3, n_frames), n_frames <= 65535.
hipError_t launch_map_arrow(const MapSeg *arrow, int n_frames, uint8_t *fb, int W, int H, hipStream_t stream, hipEvent_t start = nullptr,
                            hipEvent_t stop = nullptr);

}  // namespace dg
