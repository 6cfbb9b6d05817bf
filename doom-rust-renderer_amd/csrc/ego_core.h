// ego_core.h — the rules of the player-centred map frames as host/device inline functions: where a map vertex
// lands in a frame centred on the player, how a frame is cut into bands, what a band's owner tile holds and how it becomes RGB24.
// ego_kernels.hip runs them on the GPU, ego_host.hpp on the host (dg_ego_map_lines, dg_ego_map_host), and tests/ego/ego_host_main.cpp
// runs the kernel's three phases as a host loop over the same functions against the literal rule.
//
// The point of a map vertex (vx, vy), every operation in f32 in this order, no contraction (the units are built with -ffp-contract=off):
//     dx = vx - view.x, dy = vy - view.y
//     rotate:  r = dx * sin_a - dy * cos_a,  f = dx * cos_a + dy * sin_a        else  r = dx, f = dy
//     X = (i32) floorf((float)(W / 2) + r * scale),  Y = (i32) floorf((float)(H / 2) - f * scale)
// In contract (|vx|, |vy| <= 32768 as WAD vertices are i16, |view.x|, |view.y| <= 65536, |cos_a|, |sin_a| <= 1, scale <= 64,
// W, H <= 16384) |r|, |f| <= 2 * 98304, so |X|, |Y| <= 8192 + 64 * 196608 + rounding < 2^24: the floored value is an integer a plain
// conversion takes exactly, and map_seg_make's precondition holds for every line of every view — translated by a band's first row
// (< 16384) too.
//
// Bands.  A frame is cut into runs of whole rows of at most EGO_TILE_PX pixels: rows = max(1, EGO_TILE_PX / W), the last band of a frame
// possibly shorter; W > EGO_TILE_PX: a band is one row (at most EGO_WIDE_TILE_PX pixels).  A workgroup owns one band of one frame.
//
// The band property.  The line rule (map_core.h) depends only on coordinate differences: map_seg_point of the line translated by
// (0, -row0) gives the points of the line itself, translated.  So map_seg_make(x0, y0 - row0, x1, y1 - row0, .., W, band_rows) finds
// exactly the steps whose point lies in rows [row0, row0 + band_rows) of the frame; over the bands of a frame these ranges are disjoint
// and their union is the frame-clipped range.  tests/ego/ego_host_main.cpp checks it for every band height.
//
// The owner tile.  One uint32 per pixel of the band, 0 = no line.  A linedef's value is (index + 1) << 1 | yellow, the arrow's lies
// above every linedef's; drawing is max(), so the tile ends up with the LAST line in draw order whatever order the steps ran in.
#pragma once
#include <cmath>

#include "map_core.h"

namespace dg {

constexpr uint32_t EGO_TILE_PX = 8192u;                   // pixels of a band's tile (32 KB of LDS)
constexpr uint32_t EGO_WIDE_TILE_PX = 16384u;             // ... of a frame wider than that: one row (64 KB)
constexpr uint32_t EGO_CHUNK = 256u;                      // linedefs a workgroup examines at a time: one per lane, and its survivor list's capacity
constexpr uint32_t EGO_MAX_LINES = 65535u;                // (index + 1) << 1 | yellow stays below the arrow's value
constexpr uint32_t EGO_ROTATE = 1u, EGO_ARROW = 2u;       // DG_EGO_*
constexpr uint32_t EGO_DRAWN = 0x80000000u;               // table word: the linedef is drawn (no DONTDRAW); the low bits are its tile value
constexpr uint32_t EGO_ARROW_VALUE = 0x40000001u;         // yellow, above every linedef
constexpr uint32_t EGO_RED_RGB = 0x0000ffu, EGO_YELLOW_RGB = 0x00ffffu;   // r | g << 8 | b << 16, the map view's two colours

struct EgoView { float x, y, cos_a, sin_a; };             // what a frame's points depend on
static_assert(sizeof(EgoView) == 16, "EgoView");
struct EgoLine { float x0, y0, x1, y1; };                 // a linedef's two vertices in map space
static_assert(sizeof(EgoLine) == 16, "EgoLine");

DG_HD uint32_t ego_line_word(uint32_t index, bool yellow, bool drawn) { return drawn ? (EGO_DRAWN | ((index + 1u) << 1) | (yellow ? 1u : 0u)) : 0u; }
DG_HD uint32_t ego_value_rgb(uint32_t v) { return v == 0u ? 0u : (v & 1u) ? EGO_YELLOW_RGB : EGO_RED_RGB; }

// The point before the conversion: two floored floats (the host checks the arrow's against +-2^24 before it converts them).
DG_HD void ego_point_f(float vx, float vy, const EgoView &v, float scale, bool rotate, int32_t W, int32_t H, float &X, float &Y) {
    const float dx = vx - v.x, dy = vy - v.y;
    float r = dx, f = dy;
    if (rotate) {
        r = dx * v.sin_a - dy * v.cos_a;
        f = dx * v.cos_a + dy * v.sin_a;
    }
    X = floorf((float)(W / 2) + r * scale);
    Y = floorf((float)(H / 2) - f * scale);
}
DG_HD void ego_point(float vx, float vy, const EgoView &v, float scale, bool rotate, int32_t W, int32_t H, int32_t &X, int32_t &Y) {
    float fx, fy;
    ego_point_f(vx, vy, v, scale, rotate, W, H, fx, fy);
    X = (int32_t)fx; Y = (int32_t)fy;                     // exact: an integer within +-2^24 (see above)
}

DG_HD uint32_t ego_band_rows(uint32_t W) { return W >= EGO_TILE_PX ? 1u : EGO_TILE_PX / W; }
DG_HD uint32_t ego_bands(uint32_t W, uint32_t H) { const uint32_t r = ego_band_rows(W); return (H + r - 1u) / r; }
// Pixels per store item of the resolve phase: 16 (three 16-byte stores), 4 (three dword stores) or 1 (bytes) — the widest form at which
// every band of every frame starts on the store's boundary: the frame's pixel count and, with more than one band, a band's are multiples
// of it, and so is the slab's base address.
DG_HD uint32_t ego_store_px(uint32_t W, uint32_t H, uint64_t base) {
    const uint32_t band_px = ego_bands(W, H) > 1u ? W * ego_band_rows(W) : 0u, frame_px = W * H;
    if (base % 16u == 0u && frame_px % 16u == 0u && band_px % 16u == 0u) return 16u;
    if (base % 4u == 0u && frame_px % 4u == 0u && band_px % 4u == 0u) return 4u;
    return 1u;
}

// Does the line (x0, y0) -> (x1, y1) miss rows [row0, row0 + rows) of a frame W wide?  (Every point of a line lies in its endpoints' box.)
DG_HD bool ego_misses_band(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t W, int32_t row0, int32_t rows) {
    const int32_t xl = x0 < x1 ? x0 : x1, xh = x0 < x1 ? x1 : x0, yl = y0 < y1 ? y0 : y1, yh = y0 < y1 ? y1 : y0;
    return xh < 0 || xl >= W || yh < row0 || yl >= row0 + rows;
}

// Phase 1 for one linedef: its steps inside the band, as a segment in the band's own coordinates (count 0: nothing to draw).
DG_HD MapSeg ego_band_seg(const EgoLine &l, uint32_t value, const EgoView &v, float scale, bool rotate, int32_t W, int32_t H, int32_t row0, int32_t rows) {
    int32_t x0, y0, x1, y1;
    ego_point(l.x0, l.y0, v, scale, rotate, W, H, x0, y0);
    ego_point(l.x1, l.y1, v, scale, rotate, W, H, x1, y1);
    if (ego_misses_band(x0, y0, x1, y1, W, row0, rows)) {
        MapSeg s{};
        return s;
    }
    return map_seg_make(x0, y0 - row0, x1, y1 - row0, value, W, rows);
}

// The rows a frame-clipped segment (the arrow's, as the host sends them) can touch: [lo, hi].
DG_HD void ego_seg_rows(const MapSeg &s, int32_t &lo, int32_t &hi) {
    const int32_t dy = (s.flags & MAP_SEG_X_MAJOR) ? s.b : s.a, y1 = (s.flags & MAP_SEG_NEG_Y) ? s.y0 - dy : s.y0 + dy;
    lo = s.y0 < y1 ? s.y0 : y1; hi = s.y0 < y1 ? y1 : s.y0;
}

// Four pixels' colours (r | g << 8 | b << 16) as the 12 bytes of RGB24 they become, in three little-endian words.
DG_HD void ego_pack4_rgb(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t &o0, uint32_t &o1, uint32_t &o2) {
    o0 = c0 | (c1 << 24);
    o1 = (c1 >> 8) | (c2 << 16);
    o2 = (c2 >> 16) | (c3 << 8);
}
// ... from their tile values.
DG_HD void ego_pack4(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t &o0, uint32_t &o1, uint32_t &o2) {
    ego_pack4_rgb(ego_value_rgb(v0), ego_value_rgb(v1), ego_value_rgb(v2), ego_value_rgb(v3), o0, o1, o2);
}

}  // namespace dg
