// surface_rows_kernels.hpp — launch interface of the per-view sector flat rows (surface_rows_kernels.hip) and of the seg-walk kernel
// pairs that read them and the frames' sidedef entries (fs_surf_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "fs_frame.h"
#include "surface_rows_core.h"

namespace dg {

// dg_flat_row_fill, then (n_entries > 0) dg_flat_row_scatter on `stream`: P.rows[f][s] for every frame f < P.n_frames and sector
// s < P.n_sectors — the scene's flats, or the entry's.  A replay writes the same values again.  n_frames * n_sectors must stay
// below 2^31.  start / stop: attached to the first / last kernel's dispatch.
hipError_t launch_flat_rows(const FlatRowParams &P, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// The seg walk's second kernel argument when the batch has surfaces: the height rows and the flat rows [frame][stride], the frames'
// sidedef entries — frame f's are sides[first[f]] .. sides[first[f + 1]], sorted by sidedef — and the segs' front sidedefs; with the
// wall effects their tables.
struct FsSurf { const FsHeights *heights; const FsFlats *flats; uint32_t stride; const FsSideEntry *sides; const uint32_t *first; const int32_t *seg_side; };
struct FsSurfFx { FsFx fx; FsSurf s; };
// launch_fs / launch_fs_fx (fs_kernels.hpp) with heights, flats and sidedefs read through R: dg_sfc_segs, dg_sfc_frame /
// dg_sfc_wfx_segs, dg_sfc_wfx_frame.
hipError_t launch_fs_surf(const FsParams &P, const FsSurf &R, hipStream_t stream, hipEvent_t start = nullptr);
hipError_t launch_fs_surf_fx(const FsParams &P, const FsSurfFx &R, hipStream_t stream, hipEvent_t start = nullptr);

}  // namespace dg
