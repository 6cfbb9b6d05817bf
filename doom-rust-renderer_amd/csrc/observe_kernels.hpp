// observe_kernels.hpp — launch interface of the observation tensors on the GPU (observe_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "observe_core.h"

namespace dg {

// n_frames sources of W x H at src (RGB24 frames, or int16 distance planes, 2-byte aligned, for DG_OBS_DISTANCE) observed under d
// (obs_desc_ok) into the strided destination (obs_strides_ok, dst aligned to its element), on `stream`: 1 <= W, H <= 16384,
// n_frames >= 0.  The 16-byte kernels run when a source row is a multiple of 16 bytes and src is 16-byte aligned, the any-width ones
// otherwise.  start / stop: optional timing events attached to the first / last dispatch (kernels.hpp).
hipError_t launch_observe(const void *src, int W, int H, int n_frames, const dg_obs_desc &d, void *dst, const int64_t strides[4], hipStream_t stream,
                          hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
