// tests/floor_map/floor_map_launch_main.hip — launch_floor_map_tiles and launch_floor_seen_sectors themselves, on frame sizes the C-ABI
// refuses (under 16 pixels) and past the grid's y extent, against a host loop over the same shared functions (ego_core.h,
// floor_map_core.h: what tests/floor_map/floor_map_host_main.cpp holds against the literal rule).  tests/test_floor_map_gpu.py builds it
// together with floor_map_kernels.hip and runs it.
//   the scene   two square rooms of 256 units side by side, built here: one node (x = 256), two leaves of four segs, seven linedefs,
//               two sectors, two flats
//   65 537 frames of 4x1     two launches (65 535 + 2): every frame's view, cells and arrow are its own
//   3 frames of 8200x2       the wide tile: one row per band, dword stores
//   3 frames of 300x41       two bands, with mask rows through dg_floor_seen_sectors
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/floor_map_kernels.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("floor_map_launch_main: line %d: %s fails\n", __LINE__, #cond); return 1; } \
    } while (0)
#define HIP(call) CHECK((call) == hipSuccess)

using namespace dg;

struct World {
    std::vector<WalkNode> nodes;
    std::vector<FloorLeaf> leaves;
    std::vector<FloorSeg> segs;
    std::vector<FloorLine> flines;
    std::vector<EgoLine> lines;
    std::vector<uint32_t> words;
    std::vector<uint8_t> flats;
    std::vector<uint32_t> palette;
};

static World make_world() {
    World w;
    w.nodes = {WalkNode{256.0f, 0.0f, 0.0f, 256.0f, {~1, ~0}}};                       // left of or on x = 256: room A (leaf 0)
    const float a[4][4] = {{0, 0, 0, 256}, {0, 256, 256, 256}, {256, 256, 256, 0}, {256, 0, 0, 0}};           // each room on its segs' right
    const float b[4][4] = {{256, 0, 256, 256}, {256, 256, 512, 256}, {512, 256, 512, 0}, {512, 0, 256, 0}};
    for (const auto &s : a) w.segs.push_back(FloorSeg{s[0], s[1], s[2], s[3]});
    for (const auto &s : b) w.segs.push_back(FloorSeg{s[0], s[1], s[2], s[3]});
    w.leaves = {FloorLeaf{0u, 4u, 0}, FloorLeaf{4u, 4u, 1}};
    // linedefs: A's three walls, B's three walls, the portal (two-sided, yellow)
    const int wall_of[7] = {0, 1, 3, 5, 6, 7, 2};
    for (int k = 0; k < 7; k++) {
        const FloorSeg &s = w.segs[(size_t)wall_of[k]];
        w.lines.push_back(EgoLine{s.v1x, s.v1y, s.v2x, s.v2y});
        w.words.push_back(ego_line_word((uint32_t)k, k == 6, true));
        w.flines.push_back(k < 3 ? FloorLine{0, -1} : k < 6 ? FloorLine{1, -1} : FloorLine{0, 1});
    }
    w.flats.resize(2 * 4096);
    for (int f = 0; f < 2; f++)
        for (int y = 0; y < 64; y++)
            for (int x = 0; x < 64; x++) w.flats[(size_t)f * 4096 + (size_t)y * 64 + (size_t)x] = (uint8_t)((f ? 3 * x + 5 * y : x ^ (y * 2)) & 255);
    w.palette.resize(256);
    for (uint32_t i = 0; i < 256; i++) w.palette[i] = ((i * 7u + 1u) & 255u) | (((i * 13u + 50u) & 255u) << 8) | (((255u - i) | 1u) << 16);
    return w;
}

template <class T> static T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size() * sizeof(T), 16)) != hipSuccess) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

// One frame as dg_floor_map_tiles' phases on the host.
static void host_frame(const World &w, const FloorTables &T, int W, int H, const EgoView &v, float scale, bool rotate, const uint32_t *mask, const MapSeg *arrow,
                       const FloorCell *row, uint8_t *out) {
    std::vector<uint32_t> seen;
    if (mask) {
        seen.assign(1, 0u);
        for (size_t l = 0; l < w.flines.size(); l++)
            if (floor_seen_line(mask, (uint32_t)l))
                for (const int32_t s : {w.flines[l].front, w.flines[l].back})
                    if (s >= 0) seen[0] |= 1u << s;
    }
    const float inv = 1.0f / scale;
    const int band_rows = (int)ego_band_rows((uint32_t)W);
    for (int row0 = 0; row0 < H; row0 += band_rows) {
        const int rows = std::min(band_rows, H - row0);
        std::vector<uint32_t> tile((size_t)rows * (size_t)W, 0u);
        auto put = [&](int32_t x, int32_t y, uint32_t value) {
            if (x >= 0 && x < W && y >= 0 && y < rows) tile[(size_t)y * (size_t)W + (size_t)x] = std::max(tile[(size_t)y * (size_t)W + (size_t)x], value);
        };
        for (size_t l = 0; l < w.lines.size(); l++) {
            if (!(w.words[l] & EGO_DRAWN) || (mask && !floor_seen_line(mask, (uint32_t)l))) continue;
            const MapSeg sg = ego_band_seg(w.lines[l], w.words[l] & ~EGO_DRAWN, v, scale, rotate, W, H, row0, rows);
            for (int32_t k = 0; k < sg.count; k++) { int32_t x, y; map_seg_point(sg, (int64_t)sg.first + k, x, y); put(x, y, sg.rgb); }
        }
        if (arrow)
            for (int a = 0; a < 3; a++)
                for (int32_t k = 0; k < arrow[a].count; k++) { int32_t x, y; map_seg_point(arrow[a], (int64_t)arrow[a].first + k, x, y); put(x, y - row0, EGO_ARROW_VALUE); }
        for (size_t j = 0; j < tile.size(); j++) {
            if (tile[j] == 0u) tile[j] = floor_pixel(T, row, mask ? seen.data() : nullptr, (int32_t)(j % (size_t)W), row0 + (int32_t)(j / (size_t)W), W, H, v, inv, rotate);
            const uint32_t c = floor_value_rgb(tile[j]);
            uint8_t *const px = out + 3 * ((size_t)row0 * (size_t)W + j);
            px[0] = (uint8_t)c; px[1] = (uint8_t)(c >> 8); px[2] = (uint8_t)(c >> 16);
        }
    }
}

static int run(const World &w, const FloorTables &Th, const FloorTables &Td, const EgoLine *d_lines, const uint32_t *d_words, const FloorLine *d_flines, int W, int H, int n,
               float scale, bool rotate, bool masked, bool with_arrow, uint64_t &lit) {
    std::vector<EgoView> views((size_t)n);
    std::vector<FloorCell> cells((size_t)n * 2);
    std::vector<MapSeg> arrow((size_t)n * 3);
    std::vector<uint32_t> masks((size_t)n);
    for (int f = 0; f < n; f++) {
        const float ang = 0.37f * (float)(f % 17);
        views[(size_t)f] = EgoView{40.0f + (float)((f * 37) % 440), 20.0f + (float)((f * 11) % 220), cosf(ang), sinf(ang)};
        cells[(size_t)2 * f] = FloorCell{f % 5 == 4 ? -1 : f % 2, 0.25f + 0.25f * (float)(f % 4)};
        cells[(size_t)2 * f + 1] = FloorCell{(f + 1) % 2, f % 3 ? 1.0f : 1.5f};
        for (int a = 0; a < 3; a++) arrow[(size_t)3 * f + a] = map_seg_make(W / 2, H / 2, W / 2 + (a - 1) * (3 + f % 4), H / 2 - 2 - f % 3, EGO_YELLOW_RGB, W, H);
        masks[(size_t)f] = (uint32_t)((f * 2654435761u) >> 7) & 0x7fu;
    }
    const size_t fsz = (size_t)3 * (size_t)W * (size_t)H;
    EgoView *d_views = to_device(views);
    FloorCell *d_cells = to_device(cells);
    MapSeg *d_arrow = to_device(arrow);
    uint32_t *d_masks = to_device(masks);
    uint32_t *d_seen = nullptr;
    uint8_t *d_fb = nullptr;
    CHECK(d_views && d_cells && d_arrow && d_masks);
    HIP(hipMalloc(&d_seen, (size_t)n * 4));
    HIP(hipMalloc(&d_fb, fsz * (size_t)n));
    HIP(hipMemset(d_fb, 0x5a, fsz * (size_t)n));
    if (masked) HIP(launch_floor_seen_sectors(d_flines, (uint32_t)w.flines.size(), 2u, d_masks, 1u, d_seen, 1u, n, nullptr));
    FloorMapParams P{};
    P.E = EgoParams{d_lines, d_words, (uint32_t)w.lines.size(), d_views, with_arrow ? d_arrow : nullptr, masked ? d_masks : nullptr, 1u, scale, rotate ? 1u : 0u, W, H, d_fb, n};
    P.T = Td;
    P.cells = d_cells;
    P.seen = masked ? d_seen : nullptr;
    P.seen_words = 1u;
    P.inv = 1.0f / scale;
    HIP(launch_floor_map_tiles(P, nullptr));
    HIP(hipDeviceSynchronize());
    std::vector<uint8_t> got(fsz * (size_t)n), want(fsz);
    HIP(hipMemcpy(got.data(), d_fb, got.size(), hipMemcpyDeviceToHost));
    for (int f = 0; f < n; f++) {
        host_frame(w, Th, W, H, views[(size_t)f], scale, rotate, masked ? &masks[(size_t)f] : nullptr, with_arrow ? &arrow[(size_t)3 * f] : nullptr, &cells[(size_t)2 * f], want.data());
        if (std::memcmp(want.data(), got.data() + fsz * (size_t)f, fsz) != 0) { std::printf("floor_map_launch_main: %dx%d frame %d of %d differs\n", W, H, f, n); return 1; }
        for (uint8_t b : want) lit += b != 0;
    }
    HIP(hipFree(d_views)); HIP(hipFree(d_cells)); HIP(hipFree(d_arrow)); HIP(hipFree(d_masks)); HIP(hipFree(d_seen)); HIP(hipFree(d_fb));
    return 0;
}

int main() {
    const World w = make_world();
    const FloorTables Th{w.nodes.data(), 1u, w.leaves.data(), 2u, w.segs.data(), 8u, w.flats.data(), 2u, w.palette.data(), 2u};
    const FloorTables Td{to_device(w.nodes), 1u, to_device(w.leaves), 2u, to_device(w.segs), 8u, to_device(w.flats), 2u, to_device(w.palette), 2u};
    const EgoLine *d_lines = to_device(w.lines);
    const uint32_t *d_words = to_device(w.words);
    const FloorLine *d_flines = to_device(w.flines);
    CHECK(Td.nodes && Td.leaves && Td.segs && Td.flats && Td.palette && d_lines && d_words && d_flines);
    uint64_t lit = 0;
    CHECK(ego_bands(4u, 1u) == 1u && ego_store_px(4u, 1u, 0u) == 4u);
    if (run(w, Th, Td, d_lines, d_words, d_flines, 4, 1, 65537, 0.02f, true, false, true, lit)) return 1;
    CHECK(ego_bands(8200u, 2u) == 2u && ego_store_px(8200u, 2u, 0u) == 4u);
    if (run(w, Th, Td, d_lines, d_words, d_flines, 8200, 2, 3, 16.0f, false, false, true, lit)) return 1;
    if (run(w, Th, Td, d_lines, d_words, d_flines, 8200, 2, 2, 0.05f, true, true, false, lit)) return 1;
    CHECK(ego_bands(300u, 41u) == 2u);
    if (run(w, Th, Td, d_lines, d_words, d_flines, 300, 41, 3, 0.5f, true, true, true, lit)) return 1;
    CHECK(lit > 100000);
    // what the launcher refuses
    FloorMapParams bad{};
    bad.E.n_frames = 1; bad.E.W = 4; bad.E.H = 1;
    CHECK(launch_floor_map_tiles(bad, nullptr) == hipErrorInvalidValue);
    std::printf("floor_map_launch_main: ok (%llu lit bytes)\n", (unsigned long long)lit);
    return 0;
}
