// fs_fx_kernels.hip — the device seg walk with the scene's wall effects (dg_scene_set_wall_effects): the two kernels of
// fs_kernels.hip with FsFx in place of the default FsNoFx, so that both calls of process_seg (fs_seg_lane, fs_ph_emit) see the same effect.
// A translation unit of its own, and the effect tables in a second kernel argument rather than in FsParams, so that the plain kernels keep
// their instruction streams (one templated body shared by both files reorders operands in theirs).  dg_wfx_frame's phase sequence must
// stay that of dg_fs_frame: tests/test_wall_fx_isa.py compares the two.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "fs_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(64) void dg_wfx_segs(FsParams P, FsFx X) {
    const uint32_t si = blockIdx.x * 64u + threadIdx.x;
    if (si < P.n_segs) fs_seg_lane(P, (int)blockIdx.y, si, X);
}

// The phases of dg_fs_frame in the same order; only fs_ph_emit, which runs process_seg again for the kept parts, sees the effects.
__global__ __launch_bounds__(FS_LANES) void dg_wfx_frame(FsParams P, FsFx X) {
    __shared__ FsShared S;
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (lane == 0) fs_ph_init(S);
    __syncthreads();
    fs_ph_cand_count(P, S, f, lane);
    __syncthreads();
    fs_ph_block_sums(S, lane);
    __syncthreads();
    fs_ph_cand_stage(P, S, f, lane);
    fs_ph_first_clear(P, S, lane);
    __syncthreads();
    fs_ph_solids(P, S, f, lane);
    __syncthreads();
    fs_ph_keep(P, S, f, lane);
    __syncthreads();
    fs_ph_kept_count(P, S, f, lane);
    __syncthreads();
    fs_ph_block_sums(S, lane);
    __syncthreads();
    fs_ph_kept_place(P, S, f, lane);
    __syncthreads();
    fs_ph_emit(P, S, f, lane, X);
    __syncthreads();
    for (uint32_t base = 0; base < P.n_mobjs; base += FS_LANES) {
        FsSpriteTmp T;
        const uint32_t n_before = S.n_sprites;
        fs_ph_mobj(P, S, f, base, lane, T);
        __syncthreads();
        fs_ph_block_sums(S, lane);
        __syncthreads();
        fs_ph_mobj_emit(P, S, f, lane, T, n_before);
        __syncthreads();
    }
    fs_ph_behind(P, S, f, lane);
    fs_ph_sprite_order(S, lane);
    __syncthreads();
    fs_ph_masked_when(S, lane);
    __syncthreads();
    fs_ph_seq(P, S, f, lane);
    fs_ph_bin_clear(P, S, lane);
    __syncthreads();
    fs_ph_bin_mark(P, S, lane);
    __syncthreads();
    fs_ph_bin_count(P, S, lane);
    __syncthreads();
    if (lane == 0) fs_ph_bin_prefix(P, S, f);
    __syncthreads();
    fs_ph_bin_fill(P, S, f, lane);
    __syncthreads();
    fs_ph_clean(P, f, lane);
    if (lane == 0) fs_ph_header(P, S, f);
}

}  // namespace

hipError_t launch_fs_fx(const FsParams &P, const FsFx &X, hipStream_t stream, hipEvent_t start) {
    if (P.n_frames <= 0) return start ? hipEventRecord(start, stream) : hipSuccess;
    if (P.n_segs == 0 || !X.fx || !X.lists) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_wfx_segs, dim3((P.n_segs + 63u) / 64u, (unsigned)P.n_frames), dim3(64), 0, stream, start, nullptr, 0, P, X);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;   // each launch checked: a later success would hide it
    hipLaunchKernelGGL(dg_wfx_frame, dim3((unsigned)P.n_frames), dim3(FS_LANES), 0, stream, P, X);
    return hipGetLastError();
}

}  // namespace dg
