// mobj_fx_kernels.hpp — launch interface of the map-object thinkers' device rows (mobj_fx_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "mobj_fx.h"

namespace dg {

// dg_mobj_rows on `stream`: R.out[f][i] for every frame f < R.n_frames and map object i < R.n_mobjs.  R.out may equal R.base when
// base_stride is n_mobjs (each lane reads and writes its own element; a replay writes the same values again).
// n_frames * n_mobjs must stay below 2^31.  start: attached to the kernel's dispatch.
hipError_t launch_mobj_rows(const MfxRows &R, hipStream_t stream, hipEvent_t start = nullptr);

}  // namespace dg
