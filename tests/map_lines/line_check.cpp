// CPU check of the map view's device line-step code (doom-rust-renderer_amd/csrc/map_core.h) against the literal loop of SDL2's
// RenderDrawLineBresenham with draw_last = true.  For each line: the closed form over the clipped range [first, first + count) must
// give exactly the loop's points that lie inside the frame, in the loop's order.  Prints "ok <lines> <points>" or the first mismatch.
//   line_check exhaustive   every (dx, dy) with |dx|, |dy| <= 600 (all 8 directions), unclipped and clipped by a frame edge
//   line_check far          endpoints at +-2^24 and other far-off points, clipped to 1280x800, 40x40 and 16384x16384 frames
//   line_check random       random lines around small frames
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/map_core.h"

using dg::MapSeg;

static long long g_lines = 0, g_points = 0;

// the loop's in-frame points, in order
static void sdl_points(int64_t x0, int64_t y0, int64_t x1, int64_t y1, int W, int H, std::vector<int64_t> &out) {
    out.clear();
    const int64_t dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    int64_t n, d, inc1, inc2, xi1, xi2, yi1, yi2;
    if (dx >= dy) { n = dx + 1; d = 2 * dy - dx; inc1 = 2 * dy; inc2 = 2 * (dy - dx); xi1 = 1; xi2 = 1; yi1 = 0; yi2 = 1; }
    else { n = dy + 1; d = 2 * dx - dy; inc1 = 2 * dx; inc2 = 2 * (dx - dy); xi1 = 0; xi2 = 1; yi1 = 1; yi2 = 1; }
    if (x0 > x1) { xi1 = -xi1; xi2 = -xi2; }
    if (y0 > y1) { yi1 = -yi1; yi2 = -yi2; }
    int64_t x = x0, y = y0;
    for (int64_t i = 0; i < n; i++) {
        if (x >= 0 && x < W && y >= 0 && y < H) { out.push_back(x); out.push_back(y); }
        if (d < 0) { d += inc1; x += xi1; y += yi1; }
        else { d += inc2; x += xi2; y += yi2; }
    }
}

static bool check(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int W, int H, std::vector<int64_t> &ref) {
    sdl_points(x0, y0, x1, y1, W, H, ref);
    const MapSeg s = dg::map_seg_make(x0, y0, x1, y1, 0x123456u, W, H);
    g_lines++;
    bool ok = (size_t)s.count * 2 == ref.size() && s.first >= 0 && (int64_t)s.first + s.count <= (int64_t)s.a + 1;
    for (int32_t k = 0; ok && k < s.count; k++) {
        int32_t x, y;
        dg::map_seg_point(s, (int64_t)s.first + k, x, y);
        ok = x == ref[2 * (size_t)k] && y == ref[2 * (size_t)k + 1];
    }
    g_points += s.count;
    if (!ok) {
        std::printf("MISMATCH (%d,%d)->(%d,%d) in %dx%d: closed form first %d count %d, loop %zu points\n", x0, y0, x1, y1, W, H, s.first, s.count,
                    ref.size() / 2);
        return false;
    }
    return true;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    std::vector<int64_t> ref;
    ref.reserve(1 << 16);
    if (!std::strcmp(mode, "exhaustive")) {
        for (int dx = -600; dx <= 600; dx++)
            for (int dy = -600; dy <= 600; dy++) {
                if (!check(700, 700, 700 + dx, 700 + dy, 1401, 1401, ref)) return 1;                 // whole line inside
                if (!check(150 + dx / 3, 100 - dy / 5, 150 + dx / 3 + dx, 100 - dy / 5 + dy, 300, 200, ref)) return 1;   // leaves the frame
            }
    } else if (!std::strcmp(mode, "far")) {
        const int32_t L = 1 << 24;
        const int32_t coords[] = {-L, -L + 1, -L / 2 + 7, -1, 0, 5, 39, 399, 640, 799, 800, 1279, 1280, 16383, 16384, L / 3, L - 1, L};
        const int sizes[][2] = {{1280, 800}, {40, 40}, {16384, 16384}};
        std::vector<int32_t> pts;
        for (int32_t a : coords)
            for (int32_t b : coords) { pts.push_back(a); pts.push_back(b); }
        const size_t np = pts.size() / 2;
        // lines with at least one endpoint at +-2^24 and the other anywhere of the list, in both directions, plus a few more
        for (const auto &sz : sizes)
            for (size_t i = 0; i < np; i++)
                for (size_t j = 0; j < np; j++) {
                    const int32_t x0 = pts[2 * i], y0 = pts[2 * i + 1], x1 = pts[2 * j], y1 = pts[2 * j + 1];
                    const bool far0 = x0 == L || x0 == -L || y0 == L || y0 == -L, far1 = x1 == L || x1 == -L || y1 == L || y1 == -L;
                    if (!far0 && !far1) continue;
                    if ((i * 131 + j * 17) % 211 != 0) continue;            // a sample: each such line costs up to 2^25 loop steps
                    if (!check(x0, y0, x1, y1, sz[0], sz[1], ref)) return 1;
                }
        // lines that cross the frame from far away on either side
        const int32_t far_lines[][4] = {{-L, -L, L, L}, {L, L, -L, -L}, {-L, 400, L, 401}, {L, 401, -L, 400}, {640, -L, 641, L}, {641, L, 640, -L},
                                        {-L, L, L, -L}, {-L, -L + 3, L, L - 5}, {-L, 0, L, 800}, {0, -L, 1280, L}, {L, 5, -L, 795}};
        for (const auto &sz : sizes)
            for (const auto &l : far_lines)
                if (!check(l[0], l[1], l[2], l[3], sz[0], sz[1], ref)) return 1;
    } else if (!std::strcmp(mode, "random")) {
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&](int lo, int hi) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return lo + (int)(st % (uint64_t)(hi - lo + 1)); };
        for (int it = 0; it < 400000; it++) {
            const int W = rnd(1, 96), H = rnd(1, 96), r = rnd(1, 400);
            if (!check(rnd(-r, W + r), rnd(-r, H + r), rnd(-r, W + r), rnd(-r, H + r), W, H, ref)) return 1;
        }
    } else {
        std::fprintf(stderr, "usage: line_check exhaustive|far|random\n");
        return 2;
    }
    std::printf("ok %lld %lld\n", g_lines, g_points);
    return 0;
}
