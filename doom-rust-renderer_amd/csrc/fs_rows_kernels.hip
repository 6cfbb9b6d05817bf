// fs_rows_kernels.hip — the device seg walk with per-view sector heights (dg_view_sectors): the kernels of fs_kernels.hip
// and fs_fx_kernels.hip with the heights policy FsRowHeights in place of FsOwnHeights, so that process_seg (fs_seg_lane, fs_ph_emit)
// and the map objects (fs_ph_mobj) read the frame's row [sector] of floor and ceiling heights instead of the scene table's fields.
// The phases and their order are fs_frame.h's, the launch fs_kernels.hpp's.  A translation unit of its own, and the rows in a second
// kernel argument rather than in FsParams, so that a batch without sector entries runs kernels that never see them.
#include "fs_kernels.hpp"

namespace dg {

inline bool fs_fx_given(const FsRows &R) { return R.rows && R.stride; }
inline bool fs_fx_given(const FsRowsFx &R) { return R.rows && R.stride && fs_fx_given(R.fx); }

namespace {

// The frame's effects-and-heights policy: what fs_seg_lane and the phases are given as `fx`.
__device__ inline FsWithRows<FsNoFx> fs_rows_of(const FsRows &R, int f) { return FsWithRows<FsNoFx>{{}, FsRowHeights{R.rows + (size_t)f * R.stride}}; }
__device__ inline FsWithRows<FsFx> fs_rows_of(const FsRowsFx &R, int f) { return FsWithRows<FsFx>{R.fx, FsRowHeights{R.rows + (size_t)f * R.stride}}; }

__global__ __launch_bounds__(64) void dg_hts_segs(FsParams P, FsRows R) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, fs_rows_of(R, (int)blockIdx.y));
}

__global__ __launch_bounds__(FS_LANES) void dg_hts_frame(FsParams P, FsRows R) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const auto fx = fs_rows_of(R, f);
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

__global__ __launch_bounds__(64) void dg_hts_wfx_segs(FsParams P, FsRowsFx R) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, fs_rows_of(R, (int)blockIdx.y));
}

__global__ __launch_bounds__(FS_LANES) void dg_hts_wfx_frame(FsParams P, FsRowsFx R) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const auto fx = fs_rows_of(R, f);
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

}  // namespace

hipError_t launch_fs_rows(const FsParams &P, const FsRows &R, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_hts_segs, dg_hts_frame, P, stream, start, R); }
hipError_t launch_fs_rows_fx(const FsParams &P, const FsRowsFx &R, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_hts_wfx_segs, dg_hts_wfx_frame, P, stream, start, R); }

}  // namespace dg
