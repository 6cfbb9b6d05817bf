// fs_kernels.hpp — launch interface of the device seg walk (fs_kernels.hip, fs_fx_kernels.hip, and the pairs that read per-view rows:
// fs_rows_kernels.hip, fs_surf_kernels.hip), and what the files share.
#pragma once
#include <hip/hip_runtime_api.h>

#include "fs_frame.h"

namespace dg {

// dg_fs_segs, dg_fs_frame on `stream`.  P.flags must be zeroed (in stream order) before the launch; P.occ must be zero as well —
// dg_fs_frame leaves it so (the context zeroes it at upload and after a launch that failed half way).
// start: attached to the first kernel's dispatch.
hipError_t launch_fs(const FsParams &P, hipStream_t stream, hipEvent_t start = nullptr);
// The same with the scene's wall effects (fs_fx_kernels.hip: dg_wfx_segs, dg_wfx_frame); X.fx has one entry per seg.
hipError_t launch_fs_fx(const FsParams &P, const FsFx &X, hipStream_t stream, hipEvent_t start = nullptr);

// The seg walk's second kernel argument when the batch has height rows: the rows [frame][stride], and with the wall effects their tables.
struct FsRows { const FsHeights *rows; uint32_t stride; };
struct FsRowsFx { FsFx fx; const FsHeights *rows; uint32_t stride; };
// launch_fs / launch_fs_fx with the heights read from R.rows: dg_hts_segs, dg_hts_frame / dg_hts_wfx_segs, dg_hts_wfx_frame.
hipError_t launch_fs_rows(const FsParams &P, const FsRows &R, hipStream_t stream, hipEvent_t start = nullptr);
hipError_t launch_fs_rows_fx(const FsParams &P, const FsRowsFx &R, hipStream_t stream, hipEvent_t start = nullptr);

// The seg walk's second kernel argument when the batch has surfaces: the height rows and the flat rows [frame][stride], the frames'
// sidedef entries — frame f's are sides[first[f]] .. sides[first[f + 1]], sorted by sidedef — and the segs' front sidedefs; with the
// wall effects their tables.
struct FsSurf { const FsHeights *heights; const FsFlats *flats; uint32_t stride; const FsSideEntry *sides; const uint32_t *first; const int32_t *seg_side; };
struct FsSurfFx { FsFx fx; FsSurf s; };
// launch_fs / launch_fs_fx with heights, flats and sidedefs read through R: dg_sfc_segs, dg_sfc_frame / dg_sfc_wfx_segs, dg_sfc_wfx_frame.
hipError_t launch_fs_surf(const FsParams &P, const FsSurf &R, hipStream_t stream, hipEvent_t start = nullptr);
hipError_t launch_fs_surf_fx(const FsParams &P, const FsSurfFx &R, hipStream_t stream, hipEvent_t start = nullptr);

}  // namespace dg

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

// FS_FRAME_PHASES in a kernel: the step for the thread's own lane, then the workgroup's barrier; none after the last step.
#define FS_KERNEL_STEP(...) __VA_ARGS__; __syncthreads();
#define FS_KERNEL_LAST(...) __VA_ARGS__;

namespace dg {

inline bool fs_fx_given() { return true; }
inline bool fs_fx_given(const FsFx &X) { return X.fx && X.lists; }

// The launch of either kernel pair; x: nothing (dg_fs_*) or the FsFx (dg_wfx_*), the kernels' second argument.
template <typename... X>
hipError_t launch_fs_pair(void (*segs)(FsParams, X...), void (*frame)(FsParams, X...), const FsParams &P, hipStream_t stream, hipEvent_t start, const X &...x) {
    if (P.n_frames <= 0) return start ? hipEventRecord(start, stream) : hipSuccess;
    if (P.n_segs == 0 || !fs_fx_given(x...)) return hipErrorInvalidValue;   // (upload_fs_scene keeps a scene without segs off the seg walk)
    hipExtLaunchKernelGGL(segs, dim3((P.n_segs + 63u) / 64u, (unsigned)P.n_frames), dim3(64), 0, stream, start, nullptr, 0, P, x...);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;   // each launch checked: a later success would hide it
    hipLaunchKernelGGL(frame, dim3((unsigned)P.n_frames), dim3(FS_LANES), 0, stream, P, x...);
    return hipGetLastError();
}

}  // namespace dg
#endif
