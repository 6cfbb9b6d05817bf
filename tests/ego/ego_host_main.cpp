// tests/ego/ego_host_main.cpp WAD PATH.f32 MAP — the host side of the player-centred map frames as a stand-alone program, for a
// sanitizer build (tests/test_ego_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs
// it).  Three parts:
//   1. dg_ego_map_lines and dg_ego_map_host through the C-ABI, with buffers of exactly the sizes the contract names, against the point
//      rule and the draw rule restated here as plain loops (the literal SDL loop for every line short enough to run from its start);
//   2. the band property the kernel rests on: for every line of these frames and every band height from 1 to H — and the kernel's own
//      rows at widths 44, 64, 131, 320, 1280 and 9000 — the band-clipped step ranges of the translated line are disjoint, their union
//      is the frame-clipped range, and every step gives the frame's point;
//   3. the three phases of dg_ego_tiles as a host loop over ego_core.h's functions (tile, max, resolve in the launcher's store form)
//      against dg_ego_map_host, byte for byte.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/ego_host.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("ego_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint32_t rng32() { return (rng() << 16) ^ rng(); }

struct Case { int W, H; dg_view view; dg_ego_map params; int mask; };     // mask: 0 NULL, 1 random half, 2 all zero

static std::vector<uint32_t> mask_of(const dg_scene *s, int kind) {
    std::vector<uint32_t> m((size_t)dg_seen_words(s), 0u);
    if (kind == 1) for (uint32_t &w : m) w = rng32();
    return m;
}

// Part 1: the lines against the point rule written out here, the frame against the literal loop.
static int check_entries(const dg_scene *s, const Case &c, const std::vector<uint32_t> &mask, uint64_t &lit) {
    const dg::Scene &sc = *s->sc;
    const int W = c.W, H = c.H;
    const int n = dg_ego_map_lines(s, W, H, &c.view, &c.params, nullptr, 0);
    CHECK(n >= 0);
    std::vector<dg_map_line> lines((size_t)n);
    CHECK(dg_ego_map_lines(s, W, H, &c.view, &c.params, lines.data(), n) == n);
    dg_view v = c.view;
    dg::fill_view_trig(v);
    const bool rotate = (c.params.flags & DG_EGO_ROTATE) != 0;
    auto pt = [&](float vx, float vy, int32_t &X, int32_t &Y) {
        const float dx = vx - v.x, dy = vy - v.y;
        float r = dx, f = dy;
        if (rotate) { r = dx * v.sin_a - dy * v.cos_a; f = dx * v.cos_a + dy * v.sin_a; }
        X = (int32_t)std::floor((float)(W / 2) + r * c.params.scale);
        Y = (int32_t)std::floor((float)(H / 2) - f * c.params.scale);
    };
    size_t k = 0;
    std::vector<size_t> line_of;                           // the linedef of line k
    for (size_t l = 0; l < sc.linedefs.size(); l++) {
        const dg::LinedefRec &d = sc.linedefs[l];
        if (d.flags & 128) continue;
        CHECK(k < lines.size());
        int32_t x0, y0, x1, y1;
        pt(sc.vx[(size_t)d.v1], sc.vy[(size_t)d.v1], x0, y0);
        pt(sc.vx[(size_t)d.v2], sc.vy[(size_t)d.v2], x1, y1);
        const dg_map_line &g = lines[k++];
        CHECK(g.x0 == x0 && g.y0 == y0 && g.x1 == x1 && g.y1 == y1 && g.rgb == ((d.flags & 4) ? 0x00ffffu : 0x0000ffu));
        line_of.push_back(l);
    }
    CHECK(lines.size() == k + ((c.params.flags & DG_EGO_ARROW) ? 3u : 0u));
    const size_t bytes = (size_t)3 * (size_t)W * (size_t)H;
    std::vector<uint8_t> got(bytes, 0x5a), want(bytes, 0);
    CHECK(dg_ego_map_host(s, W, H, &c.view, &c.params, c.mask ? mask.data() : nullptr, got.data()) == DG_OK);
    for (size_t i = 0; i < lines.size(); i++) {
        if (i < k && c.mask && !((mask[line_of[i] >> 5] >> (line_of[i] & 31u)) & 1u)) continue;
        const dg_map_line &l = lines[i];
        auto put = [&](int64_t x, int64_t y) {
            if (x < 0 || y < 0 || x >= W || y >= H) return;
            uint8_t *px = want.data() + 3 * ((size_t)y * (size_t)W + (size_t)x);
            px[0] = (uint8_t)l.rgb; px[1] = (uint8_t)(l.rgb >> 8); px[2] = (uint8_t)(l.rgb >> 16);
        };
        const int64_t dx = std::llabs((int64_t)l.x1 - l.x0), dy = std::llabs((int64_t)l.y1 - l.y0);
        if (std::max(dx, dy) <= (1 << 17)) {               // the literal loop of RenderDrawLineBresenham, draw_last = true
            int64_t np, d, inc1, inc2, xi1, xi2, yi1, yi2;
            if (dx >= dy) { np = dx + 1; d = 2 * dy - dx; inc1 = 2 * dy; inc2 = 2 * (dy - dx); xi1 = 1; xi2 = 1; yi1 = 0; yi2 = 1; }
            else { np = dy + 1; d = 2 * dx - dy; inc1 = 2 * dx; inc2 = 2 * (dx - dy); xi1 = 0; xi2 = 1; yi1 = 1; yi2 = 1; }
            if (l.x0 > l.x1) { xi1 = -xi1; xi2 = -xi2; }
            if (l.y0 > l.y1) { yi1 = -yi1; yi2 = -yi2; }
            int64_t x = l.x0, y = l.y0;
            for (int64_t i2 = 0; i2 < np; i2++) {
                put(x, y);
                if (d < 0) { d += inc1; x += xi1; y += yi1; } else { d += inc2; x += xi2; y += yi2; }
            }
        } else {                                           // millions of steps: the closed form over the frame-clipped range
            const dg::MapSeg sg = dg::map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
            for (int32_t i2 = 0; i2 < sg.count; i2++) { int32_t x, y; dg::map_seg_point(sg, (int64_t)sg.first + i2, x, y); put(x, y); }
        }
    }
    CHECK(got == want);
    for (uint8_t b : got) lit += b != 0;
    return 0;
}

// Part 2 for one line and one band height.
static int check_bands(const dg_map_line &l, int W, int H, int band_rows, uint64_t &steps) {
    const dg::MapSeg full = dg::map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
    int64_t next = full.first, total = 0;                  // the bands' ranges in step order: rows rise or fall along the line
    std::vector<std::pair<int32_t, int32_t>> ranges;
    for (int row0 = 0; row0 < H; row0 += band_rows) {
        const int rows = std::min(band_rows, H - row0);
        const dg::MapSeg b = dg::map_seg_make(l.x0, l.y0 - row0, l.x1, l.y1 - row0, l.rgb, W, rows);
        CHECK(b.a == full.a && b.b == full.b && b.flags == full.flags);
        if (b.count == 0) continue;
        ranges.push_back({b.first, b.count});
        total += b.count;
        CHECK(b.first >= full.first && (int64_t)b.first + b.count <= (int64_t)full.first + full.count);
        for (int32_t i = 0; i < b.count; i++) {
            int32_t x, y, fx, fy;
            dg::map_seg_point(b, (int64_t)b.first + i, x, y);
            dg::map_seg_point(full, (int64_t)b.first + i, fx, fy);
            CHECK(x == fx && y + row0 == fy && x >= 0 && x < W && y >= 0 && y < rows);
            steps++;
        }
    }
    CHECK(total == full.count);
    std::sort(ranges.begin(), ranges.end());
    for (const auto &r : ranges) { CHECK(r.first == next); next += r.second; }       // disjoint, no gap: no point twice, none missing
    return 0;
}

// Part 3: dg_ego_tiles as a host loop.
static int check_phases(const dg_scene *s, const Case &c, const std::vector<uint32_t> &mask) {
    const dg::Scene &sc = *s->sc;
    const int W = c.W, H = c.H;
    const size_t bytes = (size_t)3 * (size_t)W * (size_t)H;
    std::vector<uint8_t> want(bytes), got(bytes, 0x5a);
    CHECK(dg_ego_map_host(s, W, H, &c.view, &c.params, c.mask ? mask.data() : nullptr, want.data()) == DG_OK);
    std::vector<dg::EgoLine> lines;
    std::vector<uint32_t> words;
    dg::ego_line_table(sc, lines, words);
    dg_view v = c.view;
    dg::fill_view_trig(v);
    const dg::EgoView ev = dg::ego_view(v);
    const bool rotate = (c.params.flags & DG_EGO_ROTATE) != 0;
    dg::MapSeg arrow[3];
    if (c.params.flags & DG_EGO_ARROW) {
        dg_map_line l[3];
        std::string err;
        CHECK(dg::ego_arrow_lines(W, H, v, c.params, l, err) == DG_OK);
        for (int k = 0; k < 3; k++) arrow[k] = dg::map_seg_make(l[k].x0, l[k].y0, l[k].x1, l[k].y1, l[k].rgb, W, H);
    }
    const uint32_t band_rows = dg::ego_band_rows((uint32_t)W), px_form = dg::ego_store_px((uint32_t)W, (uint32_t)H, 0);
    for (int row0 = 0; row0 < H; row0 += (int)band_rows) {
        const int rows = std::min((int)band_rows, H - row0);
        const uint32_t px = (uint32_t)rows * (uint32_t)W;
        CHECK(px <= (W > (int)dg::EGO_TILE_PX ? dg::EGO_WIDE_TILE_PX : dg::EGO_TILE_PX) && px % px_form == 0);
        std::vector<uint32_t> tile(px, 0u);                // exactly the band: an index outside it is the sanitizer's to report
        for (size_t base = 0; base < lines.size(); base += dg::EGO_CHUNK) {
            std::vector<dg::MapSeg> list;
            for (size_t l = base; l < std::min(lines.size(), base + dg::EGO_CHUNK); l++) {
                if (!(words[l] & dg::EGO_DRAWN) || (c.mask && !((mask[l >> 5] >> (l & 31u)) & 1u))) continue;
                const dg::MapSeg sg = dg::ego_band_seg(lines[l], words[l] & ~dg::EGO_DRAWN, ev, c.params.scale, rotate, W, H, row0, rows);
                if (sg.count > 0) list.push_back(sg);
            }
            CHECK(list.size() <= dg::EGO_CHUNK);
            for (size_t e = list.size(); e-- > 0;)         // (backwards: the order must not matter)
                for (int32_t k = 0; k < list[e].count; k++) {
                    int32_t x, y;
                    dg::map_seg_point(list[e], (int64_t)list[e].first + k, x, y);
                    CHECK(x >= 0 && x < W && y >= 0 && y < rows);
                    uint32_t &t = tile[(size_t)y * (size_t)W + (size_t)x];
                    t = std::max(t, list[e].rgb);
                }
        }
        if (c.params.flags & DG_EGO_ARROW)
            for (const dg::MapSeg &a : arrow) {
                int32_t lo, hi;
                dg::ego_seg_rows(a, lo, hi);
                for (int32_t k = 0; k < a.count; k++) {
                    int32_t x, y;
                    dg::map_seg_point(a, (int64_t)a.first + k, x, y);
                    CHECK(y >= lo && y <= hi);
                    if (a.count <= 0 || hi < row0 || lo >= row0 + rows) { CHECK(y < row0 || y >= row0 + rows); continue; }
                    y -= row0;
                    if (x >= 0 && x < W && y >= 0 && y < rows) tile[(size_t)y * (size_t)W + (size_t)x] = std::max(tile[(size_t)y * (size_t)W + (size_t)x], dg::EGO_ARROW_VALUE);
                }
            }
        uint8_t *const out = got.data() + (size_t)3 * (size_t)row0 * (size_t)W;
        for (uint32_t j = 0; j < px / px_form; j++) {
            if (px_form == 1) {
                const uint32_t rgb = dg::ego_value_rgb(tile[j]);
                out[3 * j] = (uint8_t)rgb; out[3 * j + 1] = (uint8_t)(rgb >> 8); out[3 * j + 2] = (uint8_t)(rgb >> 16);
            } else {
                for (uint32_t g = 0; g < px_form / 4; g++) {
                    const uint32_t *t = &tile[(size_t)px_form * j + 4 * g];
                    uint32_t o[3];
                    dg::ego_pack4(t[0], t[1], t[2], t[3], o[0], o[1], o[2]);
                    for (int w = 0; w < 3; w++)
                        for (int b = 0; b < 4; b++) out[(size_t)3 * px_form * j + 12 * g + 4 * w + b] = (uint8_t)(o[w] >> (8 * b));       // little-endian stores
                }
            }
        }
    }
    CHECK(got == want);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::printf("usage: ego_host_main WAD PATH.f32 MAP\n"); return 2; }
    std::ifstream wf(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(wf)), std::istreambuf_iterator<char>());
    std::ifstream pf(argv[2], std::ios::binary);
    std::vector<char> praw((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
    std::vector<float> path(praw.size() / 4);
    std::memcpy(path.data(), praw.data(), path.size() * 4);
    CHECK(!wad.empty() && path.size() >= 8 * 1000);
    dg_scene *s = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[3], &s) == DG_OK);

    const int sizes[4][2] = {{64, 40}, {44, 41}, {131, 67}, {320, 200}};
    const float scales[5] = {1.0f / 1024.0f, 0.05f, 1.0f, 8.0f, 64.0f};
    std::vector<Case> cases;
    int k = 0;
    for (const auto &sz : sizes)
        for (float scale : scales)
            for (uint32_t rot = 0; rot < 2; rot++, k++) {
                const float *r = &path[(size_t)8 * (size_t)((k * 97) % 1000)];
                dg_view v{};
                v.x = r[0]; v.y = r[1]; v.angle = r[2];
                if (k % 2) { v.cos_a = r[3]; v.sin_a = r[4]; v.cos_na = r[5]; v.sin_na = r[6]; v.trig_valid = 1; }
                cases.push_back(Case{sz[0], sz[1], v, dg_ego_map{scale, rot | ((k % 3) ? (uint32_t)DG_EGO_ARROW : 0u)}, k % 3});
            }
    uint64_t lit = 0, steps = 0;
    for (const Case &c : cases) {
        const std::vector<uint32_t> mask = mask_of(s, c.mask);
        if (check_entries(s, c, mask, lit) || check_phases(s, c, mask)) return 1;
    }
    CHECK(lit > 1000);

    // the band property: every line of these frames at every band height, and the kernel's own rows at six widths
    for (size_t ci = 0; ci < cases.size(); ci++) {
        const Case &c = cases[ci];
        const int n = dg_ego_map_lines(s, c.W, c.H, &c.view, &c.params, nullptr, 0);
        CHECK(n > 0);
        std::vector<dg_map_line> lines((size_t)n);
        CHECK(dg_ego_map_lines(s, c.W, c.H, &c.view, &c.params, lines.data(), n) == n);
        for (const dg_map_line &l : lines) {
            if (dg::ego_misses_band(l.x0, l.y0, l.x1, l.y1, c.W, 0, c.H)) { CHECK(dg::map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, c.W, c.H).count == 0); continue; }
            for (int h = 1; h <= c.H; h++)
                if (check_bands(l, c.W, c.H, h, steps)) return 1;
        }
    }
    const int widths[6][2] = {{44, 41}, {64, 40}, {131, 67}, {320, 200}, {1280, 800}, {9000, 16}};
    for (const auto &wh : widths)
        for (float scale : {0.05f, 1.0f, 64.0f}) {
            const float *r = &path[(size_t)8 * 500];
            dg_view v{};
            v.x = r[0]; v.y = r[1]; v.angle = r[2];
            const dg_ego_map p{scale, DG_EGO_ROTATE | DG_EGO_ARROW};
            const int n = dg_ego_map_lines(s, wh[0], wh[1], &v, &p, nullptr, 0);
            CHECK(n > 0);
            std::vector<dg_map_line> lines((size_t)n);
            CHECK(dg_ego_map_lines(s, wh[0], wh[1], &v, &p, lines.data(), n) == n);
            const int rows = (int)dg::ego_band_rows((uint32_t)wh[0]);
            CHECK(rows == (wh[0] > 8192 ? 1 : 8192 / wh[0]));
            for (const dg_map_line &l : lines)
                if (check_bands(l, wh[0], wh[1], rows, steps)) return 1;
        }
    CHECK(steps > 100000);

    // what is refused, with no buffer touched
    const dg_view v0{};
    const dg_ego_map bad{0.0f, 0}, good{1.0f, 0};
    uint8_t one = 7;
    CHECK(dg_ego_map_host(s, 64, 40, &v0, &bad, nullptr, &one) == DG_ERR_INVALID && one == 7);
    CHECK(dg_ego_map_host(s, 15, 40, &v0, &good, nullptr, &one) == DG_ERR_INVALID && one == 7);
    CHECK(dg_ego_map_lines(s, 64, 40, &v0, &good, nullptr, 0) > 0);
    dg_scene_free(s);
    std::printf("ego_host_main: ok (%llu lit bytes, %llu band steps)\n", (unsigned long long)lit, (unsigned long long)steps);
    return 0;
}
