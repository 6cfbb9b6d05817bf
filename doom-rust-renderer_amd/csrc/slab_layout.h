// slab_layout.h — what lies where in every slab the runtime packs, declared once.  A slab is one allocation (pinned staging and / or
// HBM) that holds several arrays, each starting on a 256-byte boundary.  context.cpp packs and points into slabs through these
// layouts, dg_create sizes the slabs by the same layouts evaluated at the capacities, and the CPU harness (tests/emul) and
// tests/slab_layout read them too: plain host C++, no HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "fs_frame.h"
#include "view_rows_core.h"
#include "walk_core.h"

namespace dg {

constexpr size_t SLAB_ALIGN = 256;
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump cursor over one slab: take() hands out the next piece's offset, end() is where the last piece ends (what has to be
// allocated or copied), next where a further piece would start.
struct SlabCursor {
    size_t next = 0, last_end = 0;
    size_t take(size_t bytes) {
        const size_t at = next;
        last_end = at + bytes;
        next = align_up(last_end, SLAB_ALIGN);
        return at;
    }
    size_t end() const { return last_end; }
};

inline size_t fe_bin_offsets(size_t W) { return (W + FE_BIN_W - 1) / FE_BIN_W + 1; }   // column-bin offsets per frame (one past the last bin)
inline size_t fe_col_groups(size_t W) { return (W + 255) / 256; }                       // dg_fe_columns: one workgroup per (frame, 256 columns)

// Host list slab (DG_FE_HOST, and the one frame redo_frame_host redoes with n_frames = 1): one H2D copy of [0, total).
struct ListLayout { size_t frames, col_off, walls, planes, spans, total; };
inline ListLayout list_layout(size_t n_frames, size_t W, size_t walls, size_t planes, size_t spans) {
    SlabCursor c;
    ListLayout L;
    L.frames = c.take(n_frames * sizeof(DevFrame));
    L.col_off = c.take(n_frames * (W + 1) * 4);
    L.walls = c.take(walls * sizeof(DevWallRec));
    L.planes = c.take(planes * sizeof(DevPlaneRec));
    L.spans = c.take(spans * sizeof(DevSpan));
    L.total = c.end();
    return L;
}

// Framebuffer slab of a bundle submission (include/doomgpu.h: dg_bundle_*) of n frames: the parts `what` names (bit 0 colour, bit 1
// depth, bit 2 labels: DG_BUNDLE_*), in this order — RGB24 colour 3nWH | int16 distance 2nWH | uint8 kind nWH | uint16 id 2nWH | uint8 cls
// nWH.  Each part starts on the slab's boundary, which also keeps the 16-bit planes aligned when 3nWH is odd.  A part that is not there
// has offset == total.
struct BundleLayout { size_t colour, distance, kind, id, cls, total; };
inline BundleLayout bundle_layout(size_t n, size_t W, size_t H, uint32_t what) {
    const size_t px = n * W * H;
    const bool colour = (what & 1u) != 0, depth = (what & 2u) != 0, labels = (what & 4u) != 0;
    SlabCursor c;
    BundleLayout L{};
    if (colour) L.colour = c.take(3 * px);
    if (depth) { L.distance = c.take(2 * px); L.kind = c.take(px); }
    if (labels) { L.id = c.take(2 * px); L.cls = c.take(px); }
    L.total = c.end();
    if (!colour) L.colour = L.total;
    if (!depth) L.distance = L.kind = L.total;
    if (!labels) L.id = L.cls = L.total;
    return L;
}
// The largest n <= max_batch whose bundle fits a framebuffer slab of max_batch RGB24 frames (0: not even one frame does).
inline size_t bundle_capacity(size_t max_batch, size_t W, size_t H, uint32_t what) {
    const size_t slab = max_batch * 3 * W * H;
    size_t lo = 0, hi = max_batch;                           // bundle_layout(lo) fits; total grows with n
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (bundle_layout(mid, W, H, what).total <= slab) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Record slab of the device column walk as the host walker packs it (DG_FE_DEVICE): one H2D copy of [0, total).
struct FeLayout { size_t frames, fframes, parts, sprites, behind, sky, bin_off, sbin_off, bins, sbins, order, total; };
inline FeLayout fe_layout(size_t n_frames, size_t W, size_t parts, size_t sprites, size_t behind, size_t skies, size_t bins, size_t sbins) {
    SlabCursor c;
    FeLayout L;
    L.frames = c.take(n_frames * sizeof(DevFrame));
    L.fframes = c.take(n_frames * sizeof(FeFrame));
    L.parts = c.take(parts * sizeof(FePart));
    L.sprites = c.take(sprites * sizeof(FeSprite));
    L.behind = c.take(behind * 4);
    L.sky = c.take(skies * 4);
    L.bin_off = c.take(n_frames * fe_bin_offsets(W) * 4);
    L.sbin_off = c.take(n_frames * fe_bin_offsets(W) * 4);
    L.bins = c.take(bins * 2);
    L.sbins = c.take(sbins * 2);
    L.order = c.take(n_frames * fe_col_groups(W) * 4);                  // dg_fe_columns' launch order
    L.total = c.end();
    return L;
}

// The seg walk's strides, which follow the scene and the frame width.
inline uint32_t fs_sprite_stride(uint32_t n_mobjs) { return std::min<uint32_t>(FS_SPRITE_CAP, std::max<uint32_t>(32u, (n_mobjs + 31u) / 32u * 32u)); }
inline uint32_t fs_sbin_stride(uint32_t sprite_stride, size_t W) { return std::min<uint32_t>(FS_SBIN_CAP, sprite_stride * (uint32_t)((W + FE_BIN_W - 1) / FE_BIN_W)); }
// Longest candidate list a frame of the scene can have (every call of every seg), in whole keep-bit words.
inline uint32_t fs_cl_row_cap(uint32_t n_segs) { return (n_segs * FS_CALLS + 31u) / 32u * 32u; }

// Record slab of the same walk as the device seg walk fills it (DG_FE_DEVICE_SEGS), with fixed per-frame strides: [0, upload) is
// copied from the host, the rest is written by dg_light_rows / dg_mobj_rows / dg_fs_*.
//   per_view_state: every frame has its own copy of the two state arrays (the kernels index them with a per-frame stride) and, with the
//   effects on, a mask of the entries its state overrides (the rows are then completed in place); without it there is one copy for the
//   batch, and the effects' kernels write per-view rows from it into the device-written part.
struct FsLayout {
    size_t frames, views, lights, mstate, lmask, mmask;                                                    // uploaded
    size_t lrows, mrows, fframes, parts, sprites, behind, sky, bin_off, sbin_off, bins, sbins;             // device-written
    size_t upload, total;
};
inline FsLayout fs_layout(size_t n_frames, size_t W, size_t n_sectors, size_t n_mobjs, bool per_view_state, bool lfx, bool mfx,
                          uint32_t sprite_stride, uint32_t sbin_stride) {
    const size_t n = n_frames, state_frames = per_view_state ? n : 1;
    SlabCursor c;
    FsLayout L;
    L.frames = c.take(n * sizeof(DevFrame));
    L.views = c.take(n * sizeof(dg_view));
    L.lights = c.take(state_frames * n_sectors * 2);
    L.mstate = c.take(state_frames * n_mobjs * 4);
    L.lmask = c.take(lfx && per_view_state ? n * ((n_sectors + 31) / 32) * 4 : 0);
    L.mmask = c.take(mfx && per_view_state ? n * ((n_mobjs + 31) / 32) * 4 : 0);
    L.lrows = c.take(lfx && !per_view_state ? n * n_sectors * 2 : 0);
    L.upload = L.lrows;
    L.mrows = c.take(mfx && !per_view_state ? n * n_mobjs * 4 : 0);
    L.fframes = c.take(n * sizeof(FeFrame));
    L.parts = c.take(n * FS_PART_CAP * sizeof(FePart));
    L.sprites = c.take(n * sprite_stride * sizeof(FeSprite));
    L.behind = c.take(n * sprite_stride * FS_BEHIND_WORDS * 4);
    L.sky = c.take(n * FS_SKY_CAP * 4);
    L.bin_off = c.take(n * fe_bin_offsets(W) * 4);
    L.sbin_off = c.take(n * fe_bin_offsets(W) * 4);
    L.bins = c.take(n * FS_BIN_CAP * 2);
    L.sbins = c.take(n * sbin_stride * 2);
    L.total = c.end();
    return L;
}

// Per-batch scratch of the seg walk, sized by the scene: the occupancy rows (zero before every walk: dg_fs_frame leaves them so), the
// candidate rows they index (never cleared) and, only for a scene whose frames can have more candidates than dg_fs_frame's shared
// memory holds (FS_CL_CAP), per frame a candidate list with its keep bits — so that no frame of the map is handed back to the host
// for its number of candidates.  cl_row_cap is FsParams::cl_row_cap: 0 when there are no such rows (cl_rows == keep_rows then).
struct FsScratchLayout { size_t occ, lite, cl_rows, keep_rows, total, zero_bytes; uint32_t cl_row_cap; };
inline FsScratchLayout fs_scratch_layout(size_t max_batch, uint32_t n_segs) {
    const uint32_t cap = fs_cl_row_cap(n_segs);
    SlabCursor c;
    FsScratchLayout L;
    L.cl_row_cap = cap > FS_CL_CAP ? cap : 0u;
    L.zero_bytes = max_batch * (size_t)fs_occ_words(n_segs) * 4;
    L.occ = c.take(L.zero_bytes);
    L.lite = c.take(max_batch * (size_t)n_segs * FS_CALLS * sizeof(uint2));
    L.cl_rows = c.take(max_batch * (size_t)L.cl_row_cap * 4);
    L.keep_rows = c.take(max_batch * (size_t)(L.cl_row_cap / 32) * 4);
    L.total = c.end();
    return L;
}

// Per-slot buffers of one kind of per-view rows through the seg walk (view_rows_core.h), sized by the scene at dg_upload_scene: the
// rows [max_batch][n_items] the row kernels write and the seg walk reads, in HBM only, and the de-duplicated entries — at the most
// one per cell — as pinned staging and as their HBM copy (two allocations of `entries` bytes: one H2D copy of what a batch has).
// cells is the capacity that follows: entries a batch can stage, and elements its rows hold.
struct ViewRowLayout { size_t cells, rows, entries; };
template <class K> ViewRowLayout view_row_layout(size_t max_batch, size_t n_items) {
    ViewRowLayout L;
    L.cells = max_batch * n_items;
    L.rows = L.cells * sizeof(typename K::Elem);
    L.entries = L.cells * sizeof(typename K::Entry);
    return L;
}
using SectorRowLayout = ViewRowLayout;
inline SectorRowLayout sector_row_layout(size_t max_batch, size_t n_sectors) { return view_row_layout<HeightRows>(max_batch, n_sectors); }

// What the per-view surfaces add to their flat rows (view_row_layout<FlatRows>, whose three fields lead here), sized likewise.
// Sidedefs (fs_core.h FsSideEntry): one table of `table` bytes, pinned and in HBM (one H2D copy of what a batch has) — [0, first_bytes)
// the frames' offsets first[frame], max_batch + 1 of them, then the frames' sorted entries one after the other, side_cap =
// kSideEntriesPerFrame x max_batch at the most: it does not grow with the map's sidedef count.
constexpr size_t kSideEntriesPerFrame = 64;
struct SurfaceLayout : ViewRowLayout { size_t side_cap, first_bytes, table; };
inline SurfaceLayout surface_layout(size_t max_batch, size_t n_sectors) {
    SurfaceLayout L;
    static_cast<ViewRowLayout &>(L) = view_row_layout<FlatRows>(max_batch, n_sectors);
    L.side_cap = kSideEntriesPerFrame * max_batch;
    L.first_bytes = align_up((max_batch + 1) * sizeof(uint32_t), 16);
    L.table = L.first_bytes + L.side_cap * sizeof(FsSideEntry);
    return L;
}

// Transient buffers of one dg_ctx_locate_walks call (walk_kernels.hip): [0, upload) is one H2D copy of the probes of all its walks,
// the rest is written by the kernels; [floors, floors + entries * 4) is the one D2H copy.  entries: one per (walk, tic), the walks' tic 0 included.
// blocks: scan workgroups, walk_scan_blocks(probes).
inline size_t walk_scan_blocks(size_t probes) { return (probes + WALK_SCAN_BLOCK - 1) / WALK_SCAN_BLOCK; }
struct WalkLayout { size_t x, y, first, end_of_tic, upload, value, last, sums, floors, total; };
inline WalkLayout walk_layout(size_t probes, size_t entries) {
    SlabCursor c;
    WalkLayout L;
    L.x = c.take(probes * 4);
    L.y = c.take(probes * 4);
    L.first = c.take(probes);
    L.end_of_tic = c.take(entries * 4);
    L.upload = c.end();
    L.value = c.take(probes * 4);
    L.last = c.take(probes * 4);
    L.sums = c.take(walk_scan_blocks(probes) * 4);
    L.floors = c.take(entries * 4);
    L.total = c.end();
    return L;
}

}  // namespace dg
