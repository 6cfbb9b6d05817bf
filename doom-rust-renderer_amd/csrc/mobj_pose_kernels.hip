// mobj_pose_kernels.hip — the seg walk's per-view map-object rows when a batch carries poses (dg_view_poses).
// dg_mobj_pose_fill: one lane per (frame, map object), numbered in one row-major index so that a map with few objects still fills its
// wavefronts; consecutive lanes store consecutive 16-byte elements.  dg_mobj_pose_place: one lane per entry; the BSP descent reads a
// node (24 B, cached: every lane starts at the root) per level, ten to thirty levels, and stores one element.  Both bodies are
// mobj_pose_core.h's, the host's too.  No LDS, no scratch, no atomics: the entries are unique per (frame, object).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "mobj_pose_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(256) void dg_mobj_pose_fill(PoseParams P) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= P.n_frames * P.n_mobjs) return;
    pose_fill(P, idx);
}

__global__ __launch_bounds__(256) void dg_mobj_pose_place(PoseParams P) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= P.n_entries) return;
    pose_place(P, e);
}

}  // namespace

hipError_t launch_mobj_poses(const PoseParams &P, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (!P.scene_rows || !P.rows || !P.nodes || !P.leaf_sector || (P.n_entries && !P.entries)) return hipErrorInvalidValue;
    if (P.n_frames == 0 || P.n_mobjs == 0 || P.root < 0) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)P.n_frames * P.n_mobjs;
    if (total >= (1ull << 31) || P.n_entries > total) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_mobj_pose_fill, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, stream, start, P.n_entries ? nullptr : stop, 0, P);
    if (P.n_entries) hipExtLaunchKernelGGL(dg_mobj_pose_place, dim3((P.n_entries + 255u) / 256u), dim3(256), 0, stream, nullptr, stop, 0, P);
    return hipGetLastError();
}

}  // namespace dg
