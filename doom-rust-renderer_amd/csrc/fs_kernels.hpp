// fs_kernels.hpp — launch interface of the device seg walk (fs_kernels.hip, fs_fx_kernels.hip), and what the two files share.
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
