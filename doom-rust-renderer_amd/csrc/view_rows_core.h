// view_rows_core.h — per-view rows: a view's own copy of one scene table, [frame][item], which the seg walk reads when a
// batch carries entries for it, as one body for the host (the list walker, the dg_slot_* row getters, the programs under tests/) and the
// device (view_rows_kernels.hip).  Two steps in stream order: every row starts as the scene's (view_row_fill, one element per lane),
// then every entry writes its item's element of its frame (view_row_scatter, one entry per lane) — the scatter depends on the fill
// only through the stream's order.  Entries are unique per (frame, item) — the host's de-duplication (frontend.hpp LatestPerIndex)
// keeps the later of two — so no two lanes write one element, and nothing here needs an atomic.
// A kind names what differs: Elem, the rows' element; Entry, one de-duplicated entry as the host ships it; Ctx, what place() needs of
// the scene besides the entry (ctx_ok: it is all there); frame() / item() of an entry; and place(), the element an entry stands for.
// The kinds: map-object poses (mobj_pose_core.h, §8m), and here sector heights (§8n) and sector flats (§8p).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fs_core.h"

namespace dg {

struct NoRowCtx {};

template <class K> struct ViewRowParams {
    const typename K::Elem *scene_rows;     // [n_items] the table as loaded
    const typename K::Entry *entries;       // [n_entries], unique per (frame, item)
    typename K::Elem *rows;                 // [n_frames][n_items]
    uint32_t n_items, n_frames, n_entries;
    typename K::Ctx ctx{};
};

// Element idx of the rows (idx < n_frames * n_items, row-major) becomes the scene's.  An element whose size is a power of two up to 16
// is taken to be aligned to its size — the tables start on a 16-byte boundary at the least (hipMalloc's 256, the host allocator's 16)
// — so that the device moves it with one load and one store (a 16-byte FsMobj: one dwordx4 each).
template <class K> DG_HD void view_row_fill(const ViewRowParams<K> &P, uint32_t idx) {
    constexpr size_t size = sizeof(typename K::Elem);
    constexpr size_t align = size <= 16 && (size & (size - 1)) == 0 ? size : alignof(typename K::Elem);
    const void *const from = __builtin_assume_aligned(P.scene_rows + idx % P.n_items, align);
    __builtin_memcpy(__builtin_assume_aligned(P.rows + idx, align), from, size);
}

// Entry e (e < n_entries) writes its item's element of its frame.
template <class K> DG_HD void view_row_scatter(const ViewRowParams<K> &P, uint32_t e) {
    const typename K::Entry en = P.entries[e];
    const int32_t frame = K::frame(en), item = K::item(en);
    if (frame < 0 || (uint32_t)frame >= P.n_frames || item < 0 || (uint32_t)item >= P.n_items) return;   // (the host has checked both)
    P.rows[(size_t)frame * P.n_items + (uint32_t)item] = K::place(P.ctx, en);
}

// Sector heights: sector `sector` of frame `frame` has these heights (both checked to fit int16).  Only the two heights travel per view:
// flats, animation lists and the sky flag stay in the scene's FsSector table, which all frames of a batch share.
struct SectorEntry { int32_t frame, sector; int16_t floor_h, ceil_h; };
static_assert(sizeof(SectorEntry) == 12, "SectorEntry layout");
// One sector's element of one view's row, from heights the caller has checked.
DG_HD void sector_row_place(FsHeights *row, int32_t sector, int32_t floor_h, int32_t ceil_h) { row[sector] = FsHeights{(int16_t)floor_h, (int16_t)ceil_h}; }
struct HeightRows {
    using Elem = FsHeights;
    using Entry = SectorEntry;
    using Ctx = NoRowCtx;
    static DG_HD bool ctx_ok(const Ctx &) { return true; }
    static DG_HD int32_t frame(const Entry &e) { return e.frame; }
    static DG_HD int32_t item(const Entry &e) { return e.sector; }
    static DG_HD Elem place(const Ctx &, const Entry &e) { return FsHeights{e.floor_h, e.ceil_h}; }
};
using SectorRowParams = ViewRowParams<HeightRows>;

// Sector flats: sector `sector` of frame `frame` has these two flat handles (both checked).  The sidedefs have no rows: a frame's
// entries stay the sorted span the seg walk searches (fs_core.h fs_side_find).
struct FlatEntry { int32_t frame, sector; FsFlats flats; };
static_assert(sizeof(FlatEntry) == 16, "FlatEntry layout");
struct FlatRows {
    using Elem = FsFlats;
    using Entry = FlatEntry;
    using Ctx = NoRowCtx;
    static DG_HD bool ctx_ok(const Ctx &) { return true; }
    static DG_HD int32_t frame(const Entry &e) { return e.frame; }
    static DG_HD int32_t item(const Entry &e) { return e.sector; }
    static DG_HD Elem place(const Ctx &, const Entry &e) { return e.flats; }
};
using FlatRowParams = ViewRowParams<FlatRows>;
DG_HD void flat_row_place(FsFlats *row, int32_t sector, FsFlats flats) { row[sector] = flats; }

}  // namespace dg
