// fs_surf_kernels.hip — the device seg walk with per-view surfaces (dg_view_surfaces): the kernels of fs_rows_kernels.hip
// with the surfaces policy FsViewSurfaces in place of FsOwnSurfaces, so that process_seg (fs_seg_lane, fs_ph_emit) reads the frame's row
// [sector] of flats and searches the frame's sorted sidedef entries for the seg's front sidedef — past the clip and back-face tests,
// where the wall effects are asked, so that only the segs that survive them search.  A batch with surfaces reads its heights through
// rows as well (the fill runs even without height entries), so there are two pairs here, not four.  The phases and their order are
// fs_frame.h's, the launch fs_kernels.hpp's.  A translation unit of its own, and the tables in a second kernel argument rather than in
// FsParams, so that a batch without surfaces runs kernels that never see them.
#include "fs_kernels.hpp"

namespace dg {

inline bool fs_fx_given(const FsSurf &R) { return R.heights && R.flats && R.stride && R.sides && R.first && R.seg_side; }
inline bool fs_fx_given(const FsSurfFx &R) { return fs_fx_given(R.s) && fs_fx_given(R.fx); }

namespace {

// The frame's effects, heights and surfaces policy: what fs_seg_lane and the phases are given as `fx`.
template <typename Fx> __device__ inline FsWithSurfaces<Fx> fs_surf_policy(const Fx &fx, const FsSurf &R, int f) {
    FsWithSurfaces<Fx> x;
    static_cast<Fx &>(x) = fx;
    x.ht = FsRowHeights{R.heights + (size_t)f * R.stride};
    const uint32_t at = R.first[f];
    x.sf = FsViewSurfaces{R.flats + (size_t)f * R.stride, R.sides + at, R.first[f + 1] - at, R.seg_side};
    return x;
}
__device__ inline FsWithSurfaces<FsNoFx> fs_surf_of(const FsSurf &R, int f) { return fs_surf_policy(FsNoFx(), R, f); }
__device__ inline FsWithSurfaces<FsFx> fs_surf_of(const FsSurfFx &R, int f) { return fs_surf_policy(R.fx, R.s, f); }

__global__ __launch_bounds__(64) void dg_sfc_segs(FsParams P, FsSurf R) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, fs_surf_of(R, (int)blockIdx.y));
}

__global__ __launch_bounds__(FS_LANES) void dg_sfc_frame(FsParams P, FsSurf R) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const auto fx = fs_surf_of(R, f);
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

__global__ __launch_bounds__(64) void dg_sfc_wfx_segs(FsParams P, FsSurfFx R) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, fs_surf_of(R, (int)blockIdx.y));
}

__global__ __launch_bounds__(FS_LANES) void dg_sfc_wfx_frame(FsParams P, FsSurfFx R) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const auto fx = fs_surf_of(R, f);
    FsSpriteTmp T;
    FS_FRAME_PHASES(FS_KERNEL_STEP, FS_KERNEL_LAST)
}

}  // namespace

hipError_t launch_fs_surf(const FsParams &P, const FsSurf &R, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_sfc_segs, dg_sfc_frame, P, stream, start, R); }
hipError_t launch_fs_surf_fx(const FsParams &P, const FsSurfFx &R, hipStream_t stream, hipEvent_t start) { return launch_fs_pair(dg_sfc_wfx_segs, dg_sfc_wfx_frame, P, stream, start, R); }

}  // namespace dg
