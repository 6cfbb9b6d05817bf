// light_fx_kernels.hpp — launch interface of the light effects' device rows (light_fx_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "light_fx.h"

namespace dg {

// dg_light_rows on `stream`: R.out[f][s] for every frame f < R.n_frames and sector s < R.n_sectors.  R.out may equal R.base when
// base_stride is n_sectors (each lane reads and writes its own element; a replay writes the same values again).
// start: attached to the kernel's dispatch.
hipError_t launch_light_rows(const LfxRows &R, hipStream_t stream, hipEvent_t start = nullptr);

}  // namespace dg
