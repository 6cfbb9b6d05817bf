// surface_rows_core.h — per-view sector flats (dg_view_surfaces): the rows [frame][sector] FsFlats the seg walk reads
// when a batch carries surface entries, as one body for the host (the list walker, dg_slot_sector_flats, tests/surfaces) and the device
// (surface_rows_kernels.hip).  The shape is sector_rows_core.h's: every row starts as the scene's flats (flat_row_fill, one 8-byte
// element per lane), then every entry writes its sector's element of its frame (flat_row_scatter, one entry per lane).  Entries are
// unique per (frame, sector) — resolve_view_surfaces keeps the later of two — so no two lanes write one element, and nothing here needs
// an atomic.  The sidedefs have no rows: a frame's entries stay the sorted span the seg walk searches (fs_core.h fs_side_find).
#pragma once
#include <stdint.h>

#include "fs_core.h"

namespace dg {

// One de-duplicated entry as the host ships it: sector `sector` of frame `frame` has these two flat handles (both checked).
struct FlatEntry { int32_t frame, sector; FsFlats flats; };
static_assert(sizeof(FlatEntry) == 16, "FlatEntry layout");

struct FlatRowParams {
    const FsFlats *scene_rows;      // [n_sectors] the flats as loaded
    const FlatEntry *entries;       // [n_entries], unique per (frame, sector)
    FsFlats *rows;                  // [n_frames][n_sectors]
    uint32_t n_sectors, n_frames, n_entries;
};

// One sector's element of one view's row.
DG_HD void flat_row_place(FsFlats *row, int32_t sector, FsFlats flats) { row[sector] = flats; }

// Element idx of the rows (idx < n_frames * n_sectors, row-major) becomes the scene's.
DG_HD void flat_row_fill(const FlatRowParams &P, uint32_t idx) { P.rows[idx] = P.scene_rows[idx % P.n_sectors]; }

// Entry e (e < n_entries) writes its sector's element of its frame.
DG_HD void flat_row_scatter(const FlatRowParams &P, uint32_t e) {
    const FlatEntry en = P.entries[e];
    if (en.frame < 0 || (uint32_t)en.frame >= P.n_frames || en.sector < 0 || (uint32_t)en.sector >= P.n_sectors) return;   // (the host has checked both)
    flat_row_place(P.rows + (size_t)en.frame * P.n_sectors, en.sector, en.flats);
}

}  // namespace dg
