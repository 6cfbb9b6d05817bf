// mobj_fx_kernels.hip — the seg walk's per-view map-object rows with the scene's state machine (dg_scene_set_mobj_thinkers,
// DESIGN.md §8d): one lane per (frame, map object) writes the object's encoded state for that view — the view's override where its
// mask bit is set, else the thinker's state at the view's tics (mobj_fx.h, the host walker's body), else the base row's value.
// The (frame, object) pairs are numbered in one row-major index, so a map with few objects still fills its wavefronts.
// No LDS, no scratch: the chain steps are read from global memory, a few words per lane.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "mobj_fx_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(256) void dg_mobj_rows(MfxRows R) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint32_t)R.n_frames * R.n_mobjs) return;
    const uint32_t f = idx / R.n_mobjs, i = idx - f * R.n_mobjs;
    int32_t v = R.base[(size_t)f * R.base_stride + i];
    const int32_t ty = R.type_of[i];
    const bool kept = R.mask && ((R.mask[(size_t)f * R.mask_words + (i >> 5)] >> (i & 31u)) & 1u);
    if (ty >= 0 && !kept) v = mfx_value(R.types[ty], R.events, R.n_events, R.chains, R.steps, fs_tics(R.views[f].timestamp));
    R.out[idx] = v;
}

}  // namespace

hipError_t launch_mobj_rows(const MfxRows &R, hipStream_t stream, hipEvent_t start) {
    if (R.n_frames <= 0 || R.n_mobjs == 0) return start ? hipEventRecord(start, stream) : hipSuccess;
    if (!R.steps || !R.chains || !R.types || !R.type_of || !R.views || !R.base || !R.out || (R.n_events && !R.events)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)R.n_frames * R.n_mobjs;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_mobj_rows, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, stream, start, nullptr, 0, R);
    return hipGetLastError();
}

}  // namespace dg
