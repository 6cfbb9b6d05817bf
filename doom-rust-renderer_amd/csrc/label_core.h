// label_core.h — the per-column and per-pixel rules of the object-label frame (include/doomgpu.h: dg_label_*), as host/device inline
// functions: dg_label_tiles and dg_label_boxes (label_kernels.hip) evaluate them per lane, dg_label_lists_host (api_scene.cpp) on the CPU.
//
// A pixel's label is the owner of the draw call that wrote it last.  Who writes is the depth frame's question and is answered with the
// same words: a wall span's texture column and row come from raster_core.h, and a transparent texel (the opacity byte) writes nothing.
// What is written differs: the owner tag of the span's draw record (owners[], parallel to the frame's walls[]) for a wall, masked wall or
// sprite column, the bare class for a floor / ceiling or the sky.  Nothing here divides: a flat's wx is never evaluated.
#pragma once
#include "raster_core.h"

namespace dg {

// include/doomgpu.h DG_LABEL_*
enum : uint32_t { LABEL_NONE = 0, LABEL_WALL = 1, LABEL_MOBJ = 2, LABEL_FLAT = 3, LABEL_SKY = 4 };

DG_HD uint32_t label_class(uint32_t tag) { return tag >> 16; }
DG_HD uint32_t label_index(uint32_t tag) { return tag & 0xffffu; }
// A tag a caller may hand over: class wall or map object, the index inside the scene's table (this keeps the box table in bounds).
DG_HD bool label_tag_ok(uint32_t tag, uint32_t n_segs, uint32_t n_mobjs) {
    return (label_class(tag) == LABEL_WALL && label_index(tag) < n_segs) || (label_class(tag) == LABEL_MOBJ && label_index(tag) < n_mobjs);
}

// One span in the form the label pixel evaluates: the rasteriser's DevRSpan (lists_dev.h) with a wall's word 3 holding the owner tag of
// its draw record where the colour path keeps the light factor (and depth keeps z).  Of a flat only word 0 (rows, kind) is ever read.
DG_HD DevRSpan label_resolve_span(const DevSpan &sp, const DevFrame &fr, const DevWallRec *walls, const uint32_t *owners, const DevScene &sc,
                                  const DevConsts &k) {
    if (sp.kind == SPAN_WALL) {
        DevRSpan o = resolve_wall_span(sp, walls[fr.wall_base + sp.rec]);
        o.w[3] = owners[fr.wall_base + sp.rec];
        return o;
    }
    if (sp.kind == SPAN_FLAT) {
        DevRSpan o;
        o.w[0] = pack_w0(sp.ctop, sp.cbot, SPAN_FLAT, false, false);
        o.w[1] = o.w[2] = o.w[3] = o.w[4] = o.w[5] = o.w[6] = o.w[7] = 0;
        return o;
    }
    return resolve_sky_span(sp, sc, k, fr);
}

DG_HD bool label_span_covers(uint32_t w0, int32_t y) { return y >= w0_ctop(w0) && y <= w0_cbot(w0); }

// Does the span write row y (one of its rows), and with which label (class << 16 | index)?  The transparency tests are the depth frame's
// (depth_core.h: depth_span_writes): the opacity byte of the texel the reference picks, for a wall with holes and for a holey sky.
DG_HD bool label_span_writes(const DevRSpan &s, const DevScene &sc, const DevConsts &k, int32_t y, uint32_t &label) {
    const uint32_t sk = w0_kind(s.w[0]);
    if (sk == SPAN_WALL) {
        if (w0_immediate(s.w[0]) && sc.texel_opq[wall_texel_offset(s.w[1], s.w[2], s.w[4], s.w[5], s.w[6], s.w[7], y)] == 0) return false;
        label = s.w[3];
        return true;
    }
    if (sk == SPAN_FLAT) {
        label = LABEL_FLAT << 16;
        return true;
    }
    if (w0_immediate(s.w[0])) {
        const uint32_t o = sky_texel_offset(s.w[2], s.w[3], sky_row(sc, k, y));
        if (o == 0xffffffffu || sc.texel_opq[o] == 0) return false;
    }
    label = LABEL_SKY << 16;
    return true;
}

// ---- boxes -----------------------------------------------------------------------------------------------------------------------------
// The box table while it is being reduced: five words per (frame, map object), all zero when nothing owns a pixel, every update an
// atomicAdd (the count) or an atomicMax of a value that is at least 1 — so one memset clears it and the order of the updates cannot
// matter.  The minima are kept as maxima of their distance from the far edge.
constexpr uint32_t LABEL_BOX_WORDS = 5;       // pixels | x1 + 1 | y1 + 1 | W - x0 | H - y0
struct LabelRawBox { uint32_t w[LABEL_BOX_WORDS]; };

// include/doomgpu.h dg_label_box from a reduced entry (x0, y0, x1, y1 = -1 when no pixel).
DG_HD void label_box_finish(const LabelRawBox &r, int32_t W, int32_t H, uint32_t &pixels, int32_t &x0, int32_t &y0, int32_t &x1, int32_t &y1) {
    pixels = r.w[0];
    if (pixels == 0) { x0 = y0 = x1 = y1 = -1; return; }
    x1 = (int32_t)r.w[1] - 1; y1 = (int32_t)r.w[2] - 1;
    x0 = W - (int32_t)r.w[3]; y0 = H - (int32_t)r.w[4];
}

}  // namespace dg
