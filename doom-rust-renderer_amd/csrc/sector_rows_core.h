// sector_rows_core.h — per-view sector heights (dg_view_sectors): the rows [frame][sector] FsHeights the seg walk reads
// when a batch moves floors or ceilings, as one body for the host (the list walker, dg_slot_sector_heights, tests/sector_heights) and
// the device (sector_rows_kernels.hip).  Two steps in stream order: every row starts as the scene's heights (sector_row_fill, one
// 4-byte element per lane), then every entry writes its sector's element of its frame (sector_row_scatter, one entry per lane).
// Entries are unique per (frame, sector) — resolve_view_sectors keeps the later of two — so no two lanes write one element, and
// nothing here needs an atomic.  Only the two heights travel per view: flats, animation lists and the sky flag stay in the scene's
// FsSector table, which all frames of a batch share.
#pragma once
#include <stdint.h>

#include "fs_core.h"

namespace dg {

// One de-duplicated entry as the host ships it: sector `sector` of frame `frame` has these heights (both checked to fit int16).
struct SectorEntry { int32_t frame, sector; int16_t floor_h, ceil_h; };
static_assert(sizeof(SectorEntry) == 12, "SectorEntry layout");

struct SectorRowParams {
    const FsHeights *scene_rows;    // [n_sectors] the heights as loaded
    const SectorEntry *entries;     // [n_entries], unique per (frame, sector)
    FsHeights *rows;                // [n_frames][n_sectors]
    uint32_t n_sectors, n_frames, n_entries;
};

// One sector's element of one view's row.
DG_HD void sector_row_place(FsHeights *row, int32_t sector, int32_t floor_h, int32_t ceil_h) { row[sector] = FsHeights{(int16_t)floor_h, (int16_t)ceil_h}; }

// Element idx of the rows (idx < n_frames * n_sectors, row-major) becomes the scene's.
DG_HD void sector_row_fill(const SectorRowParams &P, uint32_t idx) { P.rows[idx] = P.scene_rows[idx % P.n_sectors]; }

// Entry e (e < n_entries) writes its sector's element of its frame.
DG_HD void sector_row_scatter(const SectorRowParams &P, uint32_t e) {
    const SectorEntry en = P.entries[e];
    if (en.frame < 0 || (uint32_t)en.frame >= P.n_frames || en.sector < 0 || (uint32_t)en.sector >= P.n_sectors) return;   // (the host has checked both)
    sector_row_place(P.rows + (size_t)en.frame * P.n_sectors, en.sector, en.floor_h, en.ceil_h);
}

}  // namespace dg
