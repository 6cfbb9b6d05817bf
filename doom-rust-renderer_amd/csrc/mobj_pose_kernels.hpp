// mobj_pose_kernels.hpp — launch interface of the per-view map-object pose rows (mobj_pose_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "mobj_pose_core.h"

namespace dg {

// dg_mobj_pose_fill, then (n_entries > 0) dg_mobj_pose_place on `stream`: P.rows[f][i] for every frame f < P.n_frames and map object
// i < P.n_mobjs — the scene's row, or the entry's pose with the sector of its position.  A replay writes the same values again.
// n_frames * n_mobjs must stay below 2^31.  start / stop: attached to the first / last kernel's dispatch.
hipError_t launch_mobj_poses(const PoseParams &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
