// sight_kernels.hip — the line-of-sight queries on the GPU: sight_core.h's traversal, one query per lane.
// dg_sight_queries: lane i runs query i and stores its byte.  dg_sight_mobjs: a workgroup is one wavefront, one frame and 64
// consecutive map objects; the frame's viewer and height row are the wavefront's (scalar loads), a lane builds its object's query
// from the frame's pose row and runs it, and the wavefront's 64 results go out as its ballot: lanes 0 and 32 store the word of their
// 32 lanes with a plain vector store — a row is whole words, and no two wavefronts share one, so nothing needs an atomic.
// The pending far children of a lane's traversal lie in LDS, SIGHT_MAX_DEPTH 16-bit entries per lane, entry k of all lanes side by
// side (SightLaneStack with stride SIGHT_BLOCK): 8 KiB per workgroup, no scratch.  A lane touches its own column alone, so nothing
// is synchronised.  Every table is read through the vector path except what the frame makes uniform.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "sight_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(SIGHT_BLOCK) void dg_sight_queries(SightQueryParams P) {
    __shared__ int16_t stacks[SIGHT_MAX_DEPTH * SIGHT_BLOCK];
    static_assert(sizeof(stacks) == SIGHT_LDS_BYTES, "SIGHT_LDS_BYTES");
    const uint32_t i = blockIdx.x * SIGHT_BLOCK + threadIdx.x;
    if (i >= P.n) return;
    SightLaneStack stack{stacks + threadIdx.x, SIGHT_BLOCK, 0u};
    const dg_sight_query q = P.q[i];
    P.visible[i] = sight_query(P.T, q, stack);
}

__global__ __launch_bounds__(SIGHT_BLOCK) void dg_sight_mobjs(SightMobjParams P) {
    __shared__ int16_t stacks[SIGHT_MAX_DEPTH * SIGHT_BLOCK];
    static_assert(sizeof(stacks) == SIGHT_LDS_BYTES, "SIGHT_LDS_BYTES");
    const uint32_t f = blockIdx.x, lane = threadIdx.x, m = blockIdx.y * SIGHT_BLOCK + lane;
    const SightView view = P.views[f];
    const FsHeights *const row = sight_row(P.T, (int32_t)f);
    bool visible = false;
    if (m < P.n_mobjs) {
        const FsMobj pose = P.poses[(P.pose_frames > 1 ? (size_t)f * P.n_mobjs : (size_t)0) + m];
        dg_sight_query q;
        if (sight_mobj_query(P.T, (int32_t)f, view, pose, P.mobj_height[m], q)) {
            SightLaneStack stack{stacks + lane, SIGHT_BLOCK, 0u};
            visible = sight_query(P.T, q, stack, row) != 0;
        }
    }
    const uint64_t seen = __ballot(visible);              // (all 64 lanes are here: no lane has returned)
    const uint32_t word = blockIdx.y * (SIGHT_BLOCK / 32u) + (lane >> 5);
    if ((lane & 31u) == 0u && word < P.words) P.visible[(size_t)f * P.words + word] = (uint32_t)(seen >> (lane & 32u));
}

bool tables_ok(const SightTables &T) {
    return T.nodes && T.leaves && T.seg_line && T.lines && T.rows && T.n_nodes <= 32768u && T.n_leaves <= 32768u && T.row_frames >= 1u;
}

}  // namespace

hipError_t launch_sight_queries(const SightQueryParams &P, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (!tables_ok(P.T) || !P.q || !P.visible || P.n == 0 || P.n > SIGHT_MAX_QUERIES) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_sight_queries, dim3((P.n + SIGHT_BLOCK - 1u) / SIGHT_BLOCK), dim3(SIGHT_BLOCK), 0, stream, start, stop, 0, P);
    return hipGetLastError();
}

hipError_t launch_sight_mobjs(const SightMobjParams &P, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (!tables_ok(P.T) || !P.views || !P.poses || !P.mobj_height || !P.visible) return hipErrorInvalidValue;
    if (P.n_frames == 0 || P.n_mobjs == 0 || P.words != (P.n_mobjs + 31u) / 32u || P.pose_frames < 1u) return hipErrorInvalidValue;
    if ((P.T.row_frames > 1u && P.T.row_frames < P.n_frames) || (P.pose_frames > 1u && P.pose_frames < P.n_frames)) return hipErrorInvalidValue;
    const uint32_t chunks = (P.n_mobjs + SIGHT_BLOCK - 1u) / SIGHT_BLOCK;
    if (chunks > 65535u) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_sight_mobjs, dim3(P.n_frames, chunks), dim3(SIGHT_BLOCK), 0, stream, start, stop, 0, P);
    return hipGetLastError();
}

}  // namespace dg
