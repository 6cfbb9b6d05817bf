// plane_core.h — which span wrote a pixel last, and what it wrote: the one rule of the depth planes, the label planes and a bundle's
// planes (include/doomgpu.h: dg_depth_*, dg_label_*, dg_bundle_*), as host/device inline functions.  plane_tiles_body
// (plane_kernels.hip) evaluates them per lane, plane_lists_host (api_scene.cpp) on the CPU.
//
// Who writes is one question for every plane: a span writes the rows it covers, except where the texel the reference picks is
// transparent (a masked wall, a sprite, a holey sky: the opacity byte) — the pixel then keeps its earlier owner.  Only what is written
// differs: distance and kind (depth_core.h) with DEPTH, the owner's label (label_core.h) with LABELS.  Everything per column (texture
// column, the holes flag, the flat numerator) and every texel row comes from raster_core.h.
#pragma once
#include "depth_core.h"
#include "label_core.h"

namespace dg {

// include/doomgpu.h DG_BUNDLE_*: the parts a submission's framebuffer slab can hold
enum : uint32_t { BUNDLE_COLOUR = 1, BUNDLE_DEPTH = 2, BUNDLE_LABELS = 4, BUNDLE_ALL = 7 };

// One span in the form the plane pixel evaluates: the rasteriser's DevRSpan (lists_dev.h) with a wall's word 3 holding z (as i32 bits,
// DEPTH) or the owner tag of its draw record (LABELS) where the colour path keeps the light factor.  A wall needs both at once only
// with DEPTH and LABELS: the span then has a ninth word for the tag.
template <bool DEPTH, bool LABELS>
struct PlaneSpan {
    static constexpr int WORDS = DEPTH && LABELS ? 9 : 8;
    static constexpr int TAG_WORD = DEPTH && LABELS ? 8 : 3;
    uint32_t w[WORDS];
};

// DEPTH off: a wall's z and a flat's numerator are not computed, and of a flat only word 0 (rows, kind) is ever read; the flats' offset
// from the texel plane is never needed (no flat texel is read): 0.  LABELS off: owners is not read.
template <bool DEPTH, bool LABELS>
DG_HD PlaneSpan<DEPTH, LABELS> plane_resolve_span(const DevSpan &sp, const DevFrame &fr, const DevWallRec *walls, const DevPlaneRec *planes,
                                                  const uint32_t *owners, const DevScene &sc, const DevConsts &k) {
    using Span = PlaneSpan<DEPTH, LABELS>;
    DevRSpan r;
    uint32_t tag = 0;
    if (sp.kind == SPAN_WALL) {
        const DevWallRec &rec = walls[fr.wall_base + sp.rec];
        r = resolve_wall_span(sp, rec);
        if (LABELS) tag = owners[fr.wall_base + sp.rec];
        r.w[3] = DEPTH ? (uint32_t)wall_distance(sp, rec) : tag;
    } else if (sp.kind == SPAN_FLAT) {
        if (DEPTH) {
            r = resolve_flat_span(sp, planes[fr.plane_base + sp.rec], k, 0u);
        } else {
            r.w[0] = pack_w0(sp.ctop, sp.cbot, SPAN_FLAT, false, false);
            r.w[1] = r.w[2] = r.w[3] = r.w[4] = r.w[5] = r.w[6] = r.w[7] = 0;
        }
    } else {
        r = resolve_sky_span(sp, sc, k, fr);
    }
    Span o;
#pragma unroll
    for (int w = 0; w < 8; w++) o.w[w] = r.w[w];
    if (DEPTH && LABELS) o.w[Span::TAG_WORD] = tag;                      // (the ninth word: word 3 is taken)
    return o;
}

DG_HD bool plane_span_covers(uint32_t w0, int32_t y) { return y >= w0_ctop(w0) && y <= w0_cbot(w0); }

// Does the span write row y (one of its rows), and with which distance, kind and label (class << 16 | index)?  A transparent texel
// writes nothing (bitmap_render.rs:265; a sky bitmap with holes likewise).  A sky pixel the colour path leaves black because the
// reference would index outside the bitmap is a sky pixel; with a holey sky bitmap the colour path writes nothing there.  One
// transparency test for all three; a flat's wx divide only with DEPTH.  The outputs of a part the span does not carry are still set
// (far, the kind, a wall's label 0): callers that did not ask simply do not store them.
template <bool DEPTH, bool LABELS>
DG_HD bool plane_span_writes(const PlaneSpan<DEPTH, LABELS> &s, const DevScene &sc, const DevConsts &k, int32_t y, int32_t &distance, uint32_t &kind,
                             uint32_t &label) {
    const uint32_t sk = w0_kind(s.w[0]);
    if (sk == SPAN_WALL) {
        if (w0_immediate(s.w[0]) && sc.texel_opq[wall_texel_offset(s.w[1], s.w[2], s.w[4], s.w[5], s.w[6], s.w[7], y)] == 0) return false;
        distance = DEPTH ? (int32_t)s.w[3] : DEPTH_FAR;
        kind = KIND_COLUMN;
        label = LABELS ? s.w[PlaneSpan<DEPTH, LABELS>::TAG_WORD] : 0u;
        return true;
    }
    if (sk == SPAN_FLAT) {
        if (DEPTH) {
            const float vy = k.CFY - (float)y;                              // visplanes.rs:109
            distance = f32_as_i16(bits_f32(s.w[4]) / vy);                   // wx = GAME_CAMERA_FOCUS_X * wz / vy (visplanes.rs:113), `as i16` (:126)
        } else {
            distance = DEPTH_FAR;
        }
        kind = KIND_FLAT;
        label = LABEL_FLAT << 16;
        return true;
    }
    if (w0_immediate(s.w[0])) {
        const uint32_t o = sky_texel_offset(s.w[2], s.w[3], sky_row(sc, k, y));
        if (o == 0xffffffffu || sc.texel_opq[o] == 0) return false;
    }
    distance = DEPTH_FAR;
    kind = KIND_SKY;
    label = LABEL_SKY << 16;
    return true;
}

}  // namespace dg
