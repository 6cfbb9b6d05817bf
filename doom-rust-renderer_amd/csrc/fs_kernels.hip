// fs_kernels.hip — the device seg walk (DG_FE_DEVICE_SEGS): BSP visit order (inside dg_fs_segs: fs_leaf_base), per-seg processing, hidden-part culling, map objects, draw
// sequence and column bins on the GPU.  Bodies: fs_core.h (arithmetic shared with the host walker) and fs_frame.h (the per-frame
// phases and their order, also run by tests/emul on the CPU).  Integer / f32 work with short dependent chains; nothing here is a contraction (no MFMA).
// fs_fx_kernels.hip holds the same two kernels with the scene's wall effects; fs_kernels.hpp launches either pair.
#include "fs_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(64) void dg_fs_segs(FsParams P) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si);
}

// One workgroup (four wavefronts) per frame.  What the phases cost is their dependent loads, which is why the serial ones (lane 0)
// read shared memory only and meet nothing but the few candidates that survived the parallel tests.
__global__ __launch_bounds__(FS_LANES) void dg_fs_frame(FsParams P) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const FsNoFx fx;
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

}  // namespace

hipError_t launch_fs(const FsParams &P, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_fs_segs, dg_fs_frame, P, stream, start); }

}  // namespace dg
