// sector_rows_kernels.hpp — launch interface of the per-view sector height rows (sector_rows_kernels.hip) and of the seg-walk kernel
// pairs that read them (fs_rows_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "fs_frame.h"
#include "sector_rows_core.h"

namespace dg {

// dg_sector_row_fill, then (n_entries > 0) dg_sector_row_scatter on `stream`: P.rows[f][s] for every frame f < P.n_frames and sector
// s < P.n_sectors — the scene's heights, or the entry's.  A replay writes the same values again.  n_frames * n_sectors must stay
// below 2^31.  start / stop: attached to the first / last kernel's dispatch.
hipError_t launch_sector_rows(const SectorRowParams &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// The seg walk's second kernel argument when the batch has height rows: the rows [frame][stride], and with the wall effects their tables.
struct FsRows { const FsHeights *rows; uint32_t stride; };
struct FsRowsFx { FsFx fx; const FsHeights *rows; uint32_t stride; };
// launch_fs / launch_fs_fx (fs_kernels.hpp) with the heights read from R.rows: dg_hts_segs, dg_hts_frame / dg_hts_wfx_segs, dg_hts_wfx_frame.
hipError_t launch_fs_rows(const FsParams &P, const FsRows &R, hipStream_t stream, hipEvent_t start = nullptr);
hipError_t launch_fs_rows_fx(const FsParams &P, const FsRowsFx &R, hipStream_t stream, hipEvent_t start = nullptr);

}  // namespace dg
