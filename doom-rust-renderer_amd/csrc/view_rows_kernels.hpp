// view_rows_kernels.hpp — launch interface of the per-view rows (view_rows_kernels.hip): map-object poses, sector heights, sector flats.
#pragma once
#include <hip/hip_runtime_api.h>

#include "mobj_pose_core.h"
#include "view_rows_core.h"

namespace dg {

// The kind's fill kernel, then (n_entries > 0) its scatter kernel on `stream`: P.rows[f][i] for every frame f < P.n_frames and item
// i < P.n_items — the scene's element, or the entry's.  A replay writes the same values again.  n_frames * n_items must stay below
// 2^31.  start / stop: attached to the first / last kernel's dispatch.  Defined for PoseRows (dg_mobj_pose_fill / _place), HeightRows
// (dg_sector_row_fill / _scatter) and FlatRows (dg_flat_row_fill / _scatter).
template <class K> hipError_t launch_view_rows(const ViewRowParams<K> &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
