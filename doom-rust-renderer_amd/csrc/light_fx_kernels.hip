// light_fx_kernels.hip — the seg walk's per-view light rows with the scene's light effects (dg_scene_set_light_effects):
// one lane per (frame, sector) writes the sector's level for that view — the view's override where its mask bit is set, else the effect's
// level at the view's tics (light_fx.h, the host walker's body), else the base row's value.  No LDS, no scratch: the flash and fire
// tables are read from global memory, a few words per lane.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "light_fx_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(64) void dg_light_rows(LfxRows R) {
    const uint32_t s = blockIdx.x * 64u + threadIdx.x, f = blockIdx.y;
    if (s >= R.n_sectors) return;
    int16_t v = R.base[(size_t)f * R.base_stride + s];
    const int32_t ri = R.rec_of[s];
    const bool kept = R.mask && ((R.mask[(size_t)f * R.mask_words + (s >> 5)] >> (s & 31u)) & 1u);
    if (ri >= 0 && !kept) v = lfx_level(R.recs[ri], R.tab, R.seed, fs_tics(R.views[f].timestamp));
    R.out[(size_t)f * R.n_sectors + s] = v;
}

}  // namespace

hipError_t launch_light_rows(const LfxRows &R, hipStream_t stream, hipEvent_t start) {
    if (R.n_frames <= 0 || R.n_sectors == 0) return start ? hipEventRecord(start, stream) : hipSuccess;
    if (!R.recs || !R.rec_of || !R.views || !R.base || !R.out) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_light_rows, dim3((R.n_sectors + 63u) / 64u, (unsigned)R.n_frames), dim3(64), 0, stream, start, nullptr, 0, R);
    return hipGetLastError();
}

}  // namespace dg
