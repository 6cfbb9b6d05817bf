// map_core.h — line rasterisation of the 2-D map view (the reference's `viewing_map` frame, src/game.rs:245-309), as host/device
// inline functions.  map_kernels.hip runs them one lane per (line, step); the host uses them to clip every line before upload, and
// tests/map_lines/line_check.cpp compiles the same bodies on the CPU against the literal loop below.
//
// The reference draws each line with canvas.draw_line, which in SDL >= 2.0.20 ends in RenderDrawLineBresenham(.., draw_last = true):
//     dx = |x1 - x0|, dy = |y1 - y0|; the larger one (x on a tie) is the major axis, a = its extent, b = the minor extent;
//     n = a + 1 points, d = 2b - a; emit (x, y); d < 0 ? (d += 2b, step major) : (d += 2(b - a), step both); signs follow x0 > x1, y0 > y1.
// Closed form of the minor offset after i steps:  m_i = floor((2b*i + a) / (2a))   (a > 0; m_0 = 0 when a = 0).
// Proof: let r_i = 2b*i + a - 2a*m_i, so the loop's d before step i is r_i + 2b - 2a.  r_0 = a lies in [0, 2a).  If r_i + 2b >= 2a the loop
// steps the minor axis and r_{i+1} = r_i + 2b - 2a, else r_{i+1} = r_i + 2b; with b <= a both stay in [0, 2a).  So 0 <= r_i < 2a, which is the
// floor above.  m_i never decreases, so the steps whose point lies inside the frame form one range: map_seg_make finds it analytically.
#pragma once
#include <cstddef>
#include <cstring>

#include "rust_num.h"

namespace dg {

// One line of a map frame in step form, clipped to the frame: steps [first, first + count) are the points inside [0, W) x [0, H).
struct MapSeg {
    int32_t x0, y0;       // start point
    int32_t a, b;         // major / minor extent, 0 <= b <= a (endpoints within +-2^24: a < 2^26)
    int32_t first, count; // clipped step range
    uint32_t flags;       // MAP_SEG_*
    uint32_t rgb;         // r | g << 8 | b << 16
};
static_assert(sizeof(MapSeg) == 32, "MapSeg");
enum : uint32_t { MAP_SEG_X_MAJOR = 1u, MAP_SEG_NEG_X = 2u, MAP_SEG_NEG_Y = 4u };

DG_HD int64_t map_minor(int64_t a, int64_t b, int64_t i) { return a == 0 ? 0 : (2 * b * i + a) / (2 * a); }

DG_HD void map_seg_point(const MapSeg &s, int64_t i, int32_t &x, int32_t &y) {
    const int64_t m = map_minor(s.a, s.b, i);
    const int64_t dx = (s.flags & MAP_SEG_X_MAJOR) ? i : m, dy = (s.flags & MAP_SEG_X_MAJOR) ? m : i;
    x = (int32_t)(s.x0 + ((s.flags & MAP_SEG_NEG_X) ? -dx : dx));
    y = (int32_t)(s.y0 + ((s.flags & MAP_SEG_NEG_Y) ? -dy : dy));
}

DG_HD int64_t map_min64(int64_t p, int64_t q) { return p < q ? p : q; }
DG_HD int64_t map_max64(int64_t p, int64_t q) { return p > q ? p : q; }

// Step form of the line (x0, y0) -> (x1, y1) drawn into a W x H frame.  Endpoints must lie within +-2^24 (the callers check).
DG_HD MapSeg map_seg_make(int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t rgb, int32_t W, int32_t H) {
    MapSeg s;
    const int64_t dx = x1 > x0 ? (int64_t)x1 - x0 : (int64_t)x0 - x1, dy = y1 > y0 ? (int64_t)y1 - y0 : (int64_t)y0 - y1;
    const bool xmaj = dx >= dy;
    s.x0 = x0; s.y0 = y0;
    s.a = (int32_t)(xmaj ? dx : dy); s.b = (int32_t)(xmaj ? dy : dx);
    s.flags = (xmaj ? MAP_SEG_X_MAJOR : 0u) | (x0 > x1 ? MAP_SEG_NEG_X : 0u) | (y0 > y1 ? MAP_SEG_NEG_Y : 0u);
    s.rgb = rgb;
    const int64_t a = s.a, b = s.b;
    const int64_t M0 = xmaj ? x0 : y0, m0 = xmaj ? y0 : x0;                      // major / minor start
    const int64_t NM = xmaj ? W : H, Nm = xmaj ? H : W;                          // frame extent along each
    const bool negM = (s.flags & (xmaj ? MAP_SEG_NEG_X : MAP_SEG_NEG_Y)) != 0, negm = (s.flags & (xmaj ? MAP_SEG_NEG_Y : MAP_SEG_NEG_X)) != 0;
    // major: M0 +- i in [0, NM)
    int64_t lo = negM ? M0 - (NM - 1) : -M0, hi = negM ? M0 : NM - 1 - M0;
    lo = map_max64(lo, 0); hi = map_min64(hi, a);
    // minor: m0 +- m_i in [0, Nm)  <=>  m_i in [mlo, mhi]
    const int64_t mlo = negm ? m0 - (Nm - 1) : -m0, mhi = negm ? m0 : Nm - 1 - m0;
    if (mhi < 0 || mlo > b) { s.first = 0; s.count = 0; return s; }
    if (mlo > 0) lo = map_max64(lo, (2 * a * mlo - a + 2 * b - 1) / (2 * b));    // m_i >= mlo  <=>  i >= ceil((2a*mlo - a) / 2b)   (b >= mlo > 0)
    if (mhi < b) hi = map_min64(hi, (2 * a * mhi + a - 1) / (2 * b));            // m_i <= mhi  <=>  i <= floor((2a*mhi + a - 1) / 2b)  (b > mhi >= 0)
    s.first = (int32_t)lo;
    s.count = hi >= lo ? (int32_t)(hi - lo + 1) : 0;
    if (s.count == 0) s.first = 0;
    return s;
}

// The literal rule of a whole frame, on the host: black, then lines[k] (x0, y0, x1, y1, rgb: dg_map_line) for every k with keep(k), in
// order, each point of its clipped steps as RGB bytes into the W x H RGB24 frame.
template <class Line, class Keep>
inline void map_draw_lines_host(const Line *lines, size_t n, int32_t W, int32_t H, uint8_t *rgb24, Keep keep) {
    std::memset(rgb24, 0, (size_t)3 * (size_t)W * (size_t)H);
    for (size_t k = 0; k < n; k++) {
        if (!keep(k)) continue;
        const MapSeg sg = map_seg_make(lines[k].x0, lines[k].y0, lines[k].x1, lines[k].y1, lines[k].rgb, W, H);
        for (int32_t i = 0; i < sg.count; i++) {
            int32_t x, y;
            map_seg_point(sg, (int64_t)sg.first + i, x, y);
            if ((uint32_t)x >= (uint32_t)W || (uint32_t)y >= (uint32_t)H) continue;
            uint8_t *const px = rgb24 + 3 * ((size_t)y * (size_t)W + (size_t)x);
            px[0] = (uint8_t)sg.rgb; px[1] = (uint8_t)(sg.rgb >> 8); px[2] = (uint8_t)(sg.rgb >> 16);
        }
    }
}

}  // namespace dg
