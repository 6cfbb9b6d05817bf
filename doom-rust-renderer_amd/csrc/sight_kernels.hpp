// sight_kernels.hpp — launch interface of the line-of-sight kernels (sight_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "sight_core.h"

namespace dg {

constexpr uint32_t SIGHT_BLOCK = 64;                      // lanes of a workgroup of either kernel: one wavefront
constexpr uint32_t SIGHT_LDS_BYTES = SIGHT_MAX_DEPTH * SIGHT_BLOCK * 2u;      // its stacks: what either kernel declares

// dg_sight_queries' arguments: visible[i] = the result of q[i], i < n.
struct SightQueryParams {
    SightTables T;
    const dg_sight_query *q;
    uint8_t *visible;
    uint32_t n;
};
// dg_sight_mobjs' arguments: bit m of row f of visible [n_frames][words] = the result of (views[f], map object m), m < n_mobjs; the
// tail bits of a row 0.  poses [pose_frames][n_mobjs]; pose_frames 1: every frame reads the one row.
struct SightMobjParams {
    SightTables T;
    const SightView *views;
    const FsMobj *poses;
    const float *mobj_height;
    uint32_t *visible;
    uint32_t n_frames, n_mobjs, words, pose_frames;
};

// One launch each on `stream`; start / stop: attached to the kernel's dispatch.  The tables' BSP must be at most SIGHT_MAX_DEPTH deep
// and its children must fit 16 bits (the callers check both).
hipError_t launch_sight_queries(const SightQueryParams &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t launch_sight_mobjs(const SightMobjParams &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
