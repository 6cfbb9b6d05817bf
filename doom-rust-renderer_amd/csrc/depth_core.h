// depth_core.h — the per-column and per-pixel arithmetic of the depth / surface-kind frame (include/doomgpu.h: dg_depth_*), as
// host/device inline functions: dg_depth_tiles (depth_kernels.hip) evaluates them per lane, dg_depth_lists_host (api_scene.cpp) on the CPU.
//
// The depth of a pixel is the `distance: i16` the reference hands to diminish_color for it (bitmap_render.rs:190-208):
//   wall / masked wall / sprite column : z                      src/renderer/bitmap_render.rs:251,267
//   floor / ceiling                    : wx as i16              src/renderer/visplanes.rs:113,126
//   sky, nothing                       : none — 32767 ("far")   src/renderer/visplanes.rs:74 writes the palette entry as it is
// Everything per column (texture column, the holes flag, the flat numerator) and every texel row comes from raster_core.h; the only
// arithmetic stated here is z (resolve_wall_span folds it into the light factor and drops it) and the conversion of wx.
#pragma once
#include "raster_core.h"

namespace dg {

// include/doomgpu.h DG_KIND_*: the draw call that wrote the pixel last
enum : uint32_t { KIND_NONE = 0, KIND_COLUMN = 1, KIND_FLAT = 2, KIND_SKY = 3 };
constexpr int32_t DEPTH_FAR = 32767;          // the distance of a pixel nothing with a distance wrote

// z of bitmap_render.rs:251 — resolve_wall_span's expression, operand for operand.
DG_HD int32_t wall_distance(const DevSpan &sp, const DevWallRec &r) {
    float ax = (float)((int32_t)sp.x - r.start_x) / r.dxf;
    float oma = 1.0f - ax;
    float den = oma * r.C + ax * r.D;
    return f32_as_i16((oma + ax) / den);
}

// One span in the form the depth pixel evaluates: the rasteriser's DevRSpan (lists_dev.h) with a wall's word 3 holding z (as i32 bits)
// where the colour path keeps the light factor.  The flats' offset from the texel plane is not needed (no flat texel is read): 0.
DG_HD DevRSpan depth_resolve_span(const DevSpan &sp, const DevFrame &fr, const DevWallRec *walls, const DevPlaneRec *planes,
                                  const DevScene &sc, const DevConsts &k) {
    if (sp.kind == SPAN_WALL) {
        const DevWallRec &r = walls[fr.wall_base + sp.rec];
        DevRSpan o = resolve_wall_span(sp, r);
        o.w[3] = (uint32_t)wall_distance(sp, r);
        return o;
    }
    if (sp.kind == SPAN_FLAT) return resolve_flat_span(sp, planes[fr.plane_base + sp.rec], k, 0u);
    return resolve_sky_span(sp, sc, k, fr);
}

DG_HD bool depth_span_covers(uint32_t w0, int32_t y) { return y >= w0_ctop(w0) && y <= w0_cbot(w0); }

// Does the span write row y (one of its rows), and with which kind and distance?  A transparent texel writes nothing
// (bitmap_render.rs:265; a sky bitmap with holes likewise) and the pixel keeps its earlier owner.  A sky pixel the colour path leaves
// black because the reference would index outside the bitmap is a sky pixel; with a holey sky bitmap the colour path writes nothing there.
DG_HD bool depth_span_writes(const DevRSpan &s, const DevScene &sc, const DevConsts &k, int32_t y, int32_t &distance, uint32_t &kind) {
    const uint32_t sk = w0_kind(s.w[0]);
    if (sk == SPAN_WALL) {
        if (w0_immediate(s.w[0]) && sc.texel_opq[wall_texel_offset(s.w[1], s.w[2], s.w[4], s.w[5], s.w[6], s.w[7], y)] == 0) return false;
        distance = (int32_t)s.w[3];
        kind = KIND_COLUMN;
        return true;
    }
    if (sk == SPAN_FLAT) {
        const float vy = k.CFY - (float)y;                              // visplanes.rs:109
        distance = f32_as_i16(bits_f32(s.w[4]) / vy);                   // wx = GAME_CAMERA_FOCUS_X * wz / vy (visplanes.rs:113), `as i16` (:126)
        kind = KIND_FLAT;
        return true;
    }
    if (w0_immediate(s.w[0])) {
        const uint32_t o = sky_texel_offset(s.w[2], s.w[3], sky_row(sc, k, y));
        if (o == 0xffffffffu || sc.texel_opq[o] == 0) return false;
    }
    distance = DEPTH_FAR;
    kind = KIND_SKY;
    return true;
}

}  // namespace dg
