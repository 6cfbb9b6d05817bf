// overlay_plan.hpp — a call's screen pictures (include/doomgpu.h: items[], first[n + 1]) checked as a whole and resolved into what the
// host twin and the kernel walk (overlay_core.h): the items that cover a pixel, in list order, and per frame the
// disjoint rectangles that hold them, cut into records of at most OVL_TILES_PER_RECT tiles.  Host only.
//
// The rectangles of a frame are its bands: between two neighbouring top / bottom edges of its items, the span from the leftmost to the
// rightmost item that crosses the band (a status bar, a weapon above it and a crosshair give three).  A frame with more than
// OVL_BAND_ITEMS items takes its items' one bounding rectangle instead, so that the planning stays linear in the items.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "overlay_core.h"

namespace dg {

constexpr uint32_t OVL_BAND_ITEMS = 64;

struct OvlPlan {
    std::vector<OvlItem> items;
    std::vector<OvlRect> rects;
    uint32_t max_tiles = 0;          // the most tiles one record names
};

// What every overlay call checks before it draws anything; nullptr, or what is wrong.
inline const char *overlay_check(int32_t n_pictures, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first) {
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return "width/height must be in [1, 16384]";
    if (n_frames < 0) return "bad frame count";
    if (n_frames == 0) return nullptr;
    if (!first) return "null argument";
    if (first[0] != 0u) return "first[0] must be 0";
    for (int f = 0; f < n_frames; f++)
        if (first[f + 1] < first[f]) return "first[] must be non-decreasing";
    const uint32_t n = first[n_frames];
    if (n > 0 && !items) return "null argument";
    for (uint32_t i = 0; i < n; i++)
        if (!ovl_item_ok(items[i], n_pictures))
            return "screen picture: a picture handle of the scene, scales in 1..16, light_level in 0..255, x and y within +-(1 << 20), no unknown flag bits";
    return nullptr;
}

inline void overlay_emit_rect(OvlPlan &plan, uint32_t frame, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t item0, uint32_t item1) {
    const uint32_t tiles_x = ((uint32_t)(x1 - x0) + OVL_TILE_W - 1u) / OVL_TILE_W, tiles_y = ((uint32_t)(y1 - y0) + OVL_TILE_H - 1u) / OVL_TILE_H;
    const uint32_t total = tiles_x * tiles_y;                    // <= 256 * 1024
    for (uint32_t t = 0; t < total; t += OVL_TILES_PER_RECT) {
        const uint32_t n = std::min(OVL_TILES_PER_RECT, total - t);
        plan.rects.push_back(OvlRect{frame, (uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1, item0, item1, t, n, tiles_x});
        plan.max_tiles = std::max(plan.max_tiles, n);
    }
}

// The rectangles of one frame whose resolved items are plan.items[item0, item1).
inline void overlay_frame_rects(OvlPlan &plan, uint32_t frame, uint32_t item0, uint32_t item1) {
    if (item0 == item1) return;
    const OvlItem *const it = plan.items.data();
    if (item1 - item0 > OVL_BAND_ITEMS) {
        int32_t x0 = it[item0].x0, y0 = it[item0].y0, x1 = it[item0].x1, y1 = it[item0].y1;
        for (uint32_t k = item0 + 1; k < item1; k++) { x0 = std::min(x0, it[k].x0); y0 = std::min(y0, it[k].y0); x1 = std::max(x1, it[k].x1); y1 = std::max(y1, it[k].y1); }
        overlay_emit_rect(plan, frame, x0, y0, x1, y1, item0, item1);
        return;
    }
    int32_t edges[2 * OVL_BAND_ITEMS];
    uint32_t ne = 0;
    for (uint32_t k = item0; k < item1; k++) { edges[ne++] = it[k].y0; edges[ne++] = it[k].y1; }
    std::sort(edges, edges + ne);
    ne = (uint32_t)(std::unique(edges, edges + ne) - edges);
    struct Band { int32_t x0, y0, x1, y1; uint32_t k0, k1; } open{0, 0, 0, 0, 0, 0};
    bool have = false;
    for (uint32_t e = 0; e + 1 < ne; e++) {
        const int32_t ya = edges[e], yb = edges[e + 1];
        Band b{0, ya, 0, yb, 0, 0};
        bool any = false;
        for (uint32_t k = item0; k < item1; k++) {
            if (it[k].y0 > ya || it[k].y1 < yb) continue;
            if (!any) { b.x0 = it[k].x0; b.x1 = it[k].x1; b.k0 = k; any = true; }
            b.x0 = std::min(b.x0, it[k].x0); b.x1 = std::max(b.x1, it[k].x1); b.k1 = k + 1;
        }
        if (any && have && open.y1 == ya && open.x0 == b.x0 && open.x1 == b.x1) {           // the band goes on: one rectangle
            open.y1 = yb; open.k0 = std::min(open.k0, b.k0); open.k1 = std::max(open.k1, b.k1);
            continue;
        }
        if (have) overlay_emit_rect(plan, frame, open.x0, open.y0, open.x1, open.y1, open.k0, open.k1);
        open = b; have = any;
    }
    if (have) overlay_emit_rect(plan, frame, open.x0, open.y0, open.x1, open.y1, open.k0, open.k1);
}

// The plan of a call that overlay_check accepted, on pictures[]: frame numbers count from 0.
inline void overlay_plan(const OvlPicture *pictures, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first, OvlPlan &plan) {
    plan = OvlPlan{};
    for (int f = 0; f < n_frames; f++) {
        const uint32_t item0 = (uint32_t)plan.items.size();
        for (uint32_t i = first[f]; i < first[f + 1]; i++) {
            OvlItem o;
            if (ovl_resolve(items[i], pictures[items[i].picture], width, height, o)) plan.items.push_back(o);
        }
        overlay_frame_rects(plan, (uint32_t)f, item0, (uint32_t)plan.items.size());
    }
}

}  // namespace dg
