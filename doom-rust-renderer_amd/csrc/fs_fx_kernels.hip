// fs_fx_kernels.hip — the device seg walk with the scene's wall effects (dg_scene_set_wall_effects): the two kernels of
// fs_kernels.hip with FsFx in place of FsNoFx, so that both calls of process_seg (fs_seg_lane, fs_ph_emit) see the same effect.  The
// phases and their order are fs_frame.h's, the launch fs_kernels.hpp's: only the effect differs.  A translation unit of its own, and the
// effect tables in a second kernel argument rather than in FsParams, so that a scene without effects runs kernels that never see them.
#include "fs_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(64) void dg_wfx_segs(FsParams P, FsFx X) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, X);
}

// Only fs_ph_emit, which runs process_seg again for the kept parts, sees the effects.
__global__ __launch_bounds__(FS_LANES) void dg_wfx_frame(FsParams P, FsFx fx) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

}  // namespace

hipError_t launch_fs_fx(const FsParams &P, const FsFx &X, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_wfx_segs, dg_wfx_frame, P, stream, start, X); }

}  // namespace dg
