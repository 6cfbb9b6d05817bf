// bundle_core.h — the per-column and per-pixel rule of a bundle submission (include/doomgpu.h: dg_bundle_*), as host/device inline
// functions: dg_bundle_tiles (bundle_kernels.hip) evaluates them per lane, dg_bundle_lists_host (api_scene.cpp) on the CPU.
//
// A bundle asks for the depth planes, the label planes or both of the same spans.  Who writes a pixel is one question for both — the
// transparency test of depth_core.h / label_core.h, run once — and only what is written differs.  Nothing is restated here that those two
// state: z is depth_core.h's wall_distance, the tags and the box words are label_core.h's.  A wall span needs z and its owner tag at
// once, and both cores keep theirs in word 3, so the bundle's span has a ninth word for the tag.
#pragma once
#include "depth_core.h"
#include "label_core.h"

namespace dg {

// include/doomgpu.h DG_BUNDLE_*
enum : uint32_t { BUNDLE_COLOUR = 1, BUNDLE_DEPTH = 2, BUNDLE_LABELS = 4, BUNDLE_ALL = 7 };

constexpr int BUNDLE_WORDS = 9;               // DevRSpan's eight, word 3 of a wall = z as in depth_core.h; word 8 = the wall's owner tag
struct BundleRSpan { uint32_t w[BUNDLE_WORDS]; };

// One span in the form the bundle pixel evaluates.  DEPTH off: a wall's z and a flat's numerator are not computed (label_resolve_span's
// flat); LABELS off: owners is not read and word 8 is 0.
template <bool DEPTH, bool LABELS>
DG_HD BundleRSpan bundle_resolve_span(const DevSpan &sp, const DevFrame &fr, const DevWallRec *walls, const DevPlaneRec *planes, const uint32_t *owners,
                                      const DevScene &sc, const DevConsts &k) {
    DevRSpan r;
    uint32_t tag = 0;
    if (sp.kind == SPAN_WALL) {
        const DevWallRec &rec = walls[fr.wall_base + sp.rec];
        r = resolve_wall_span(sp, rec);
        r.w[3] = DEPTH ? (uint32_t)wall_distance(sp, rec) : 0u;
        if (LABELS) tag = owners[fr.wall_base + sp.rec];
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
    BundleRSpan o;
#pragma unroll
    for (int w = 0; w < 8; w++) o.w[w] = r.w[w];
    o.w[8] = tag;
    return o;
}

DG_HD bool bundle_span_covers(uint32_t w0, int32_t y) { return y >= w0_ctop(w0) && y <= w0_cbot(w0); }

// Does the span write row y (one of its rows), and with which distance, kind (depth_core.h) and label (label_core.h)?  One transparency
// test for all three; a flat's wx divide only with DEPTH.  Without DEPTH distance and kind are still set (far / the kind): callers that
// did not ask simply do not store them.
template <bool DEPTH>
DG_HD bool bundle_span_writes(const BundleRSpan &s, const DevScene &sc, const DevConsts &k, int32_t y, int32_t &distance, uint32_t &kind, uint32_t &label) {
    const uint32_t sk = w0_kind(s.w[0]);
    if (sk == SPAN_WALL) {
        if (w0_immediate(s.w[0]) && sc.texel_opq[wall_texel_offset(s.w[1], s.w[2], s.w[4], s.w[5], s.w[6], s.w[7], y)] == 0) return false;
        distance = (int32_t)s.w[3];
        kind = KIND_COLUMN;
        label = s.w[8];
        return true;
    }
    if (sk == SPAN_FLAT) {
        if (DEPTH) {
            const float vy = k.CFY - (float)y;                              // depth_core.h: depth_span_writes
            distance = f32_as_i16(bits_f32(s.w[4]) / vy);
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
