// tests/floor_map/floor_map_host_main.cpp WAD PATH.f32 MAP — the host side of the floor-textured map frames as a stand-alone program, for
// a sanitizer build (tests/test_floor_map_host.py builds it with -fsanitize=address,undefined together with the library's host sources
// and runs it).  For frames of 5x3, 131x67, 1x1 and 8200x2 (below the C-ABI's 16 pixels, so through the shared functions themselves):
//   1. the literal rule restated here as plain loops over the scene's own records (NODES, SSECTORS, SEGS as loaded, not the flattened
//      tables): the lines drawn in order, then every black pixel through the five steps;
//   2. dg_floor_map_tiles' phases as a host loop over ego_core.h's and floor_map_core.h's functions — owner tile, lines and arrow by
//      max, the floor phase into the words that stayed 0, the resolve in the launcher's store form — on a heap tile of exactly the
//      band's size and a heap frame of exactly 3 W H bytes, against 1. byte for byte;
//   3. at 131x67, dg_floor_map_host through the C-ABI against 1., and what it refuses, with the output untouched;
//   4. the table sets of floor_map_tables.h (no nodes, a leaf without a sector, a leaf without segs, a chain of 200 partitions, every
//      index the rule must refuse and its control) through floor_map_core.h's functions over heap tables of exactly the stated counts:
//      a refused index gives background, and where no index is out of range the frame equals a literal descent written here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/floor_map_host.hpp"
#include "floor_map_tables.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("floor_map_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint32_t rng32() { return (rng() << 16) ^ rng(); }

struct Case { int W, H; dg_view view; dg_ego_map params; int mask; bool entries; };     // mask: 0 NULL, 1 random half, 2 all zero

// The view's inputs of a case with entries: two light entries and one flat entry on the sector under the view.
struct Inputs {
    std::vector<dg_sector_light> lights;
    std::vector<dg_sector_flats> flats;
    dg_view_state state{};
    dg_view_surfaces surfaces{};
};
static void inputs_of(const dg::Scene &sc, const Case &c, Inputs &in) {
    in = Inputs{};
    if (!c.entries) return;
    const int here = std::max(0, sc.sector_from_vertex(c.view.x, c.view.y));
    const int other = (here + 1) % (int)sc.sectors.size();
    in.lights = {{here, 96}, {other, 300}, {here, 144}};
    in.flats = {{other, sc.fs_flats[(size_t)here].floor, sc.fs_flats[(size_t)other].ceil}};
    in.state = dg_view_state{in.lights.data(), (uint32_t)in.lights.size(), nullptr, 0u};
    in.surfaces = dg_view_surfaces{nullptr, 0u, in.flats.data(), (uint32_t)in.flats.size()};
}

// Part 1: the literal rule.  cells: the view's row (floor_view_cells, held against the numpy model by the Python tier).
static int literal_frame(const dg::Scene &sc, const Case &c, const dg_view &v, const uint32_t *mask, const std::vector<dg::FloorCell> &cells, std::vector<uint8_t> &out) {
    const int W = c.W, H = c.H;
    std::vector<dg_map_line> lines;
    std::string err;
    CHECK(dg::ego_frame_lines(sc, W, H, v, c.params, mask, lines, err) == DG_OK);
    dg::map_draw_lines_host(lines.data(), lines.size(), W, H, out.data(), [](size_t) { return true; });
    std::vector<uint8_t> shown(sc.sectors.size(), mask ? 0 : 1);
    if (mask)
        for (size_t l = 0; l < sc.linedefs.size(); l++)
            if ((mask[l >> 5] >> (l & 31u)) & 1u)
                for (const int32_t sd : {sc.linedefs[l].front, sc.linedefs[l].back})
                    if (sd >= 0) shown[(size_t)sc.sidedefs[(size_t)sd].sector] = 1;
    const float inv = 1.0f / c.params.scale;
    const bool rotate = (c.params.flags & DG_EGO_ROTATE) != 0;
    for (int Y = 0; Y < H; Y++)
        for (int X = 0; X < W; X++) {
            uint8_t *const px = out.data() + 3 * ((size_t)Y * (size_t)W + (size_t)X);
            if (px[0] | px[1] | px[2]) continue;
            const float r = ((float)(X - W / 2) + 0.5f) * inv, f = ((float)(H / 2 - Y) - 0.5f) * inv;
            const float dx = rotate ? r * v.sin_a + f * v.cos_a : r, dy = rotate ? f * v.sin_a - r * v.cos_a : f;
            const float mx = v.x + dx, my = v.y + dy;
            int leaf = 0;
            if (!sc.nodes.empty()) {
                int ni = (int)sc.nodes.size() - 1;
                for (;;) {
                    const dg::NodeRec &n = sc.nodes[(size_t)ni];
                    const float v2x = n.x + n.dx, v2y = n.y + n.dy;
                    const float ax = mx - n.x, ay = my - n.y, bx = v2x - n.x, by = v2y - n.y;
                    const int child = (uint16_t)(ax * by - ay * bx <= 0.0f ? n.lchild : n.rchild);
                    if (child & 0x8000) { leaf = child & 0x7fff; break; }
                    ni = child;
                }
            }
            const dg::SubSectorRec &ss = sc.subsectors[(size_t)leaf];
            int sector = -1;
            bool behind = false;
            for (int k = 0; k < ss.count; k++) {
                const dg::SegRec &sg = sc.segs[(size_t)(ss.first + k)];
                const int sd = sg.direction ? sc.linedefs[(size_t)sg.linedef].back : sc.linedefs[(size_t)sg.linedef].front;
                if (sector < 0 && sd >= 0) sector = sc.sidedefs[(size_t)sd].sector;
                const float v1x = sc.vx[(size_t)sg.v1], v1y = sc.vy[(size_t)sg.v1], v2x = sc.vx[(size_t)sg.v2], v2y = sc.vy[(size_t)sg.v2];
                const float ax = mx - v1x, ay = my - v1y, bx = v2x - v1x, by = v2y - v1y;
                behind |= ax * by - ay * bx < 0.0f;
            }
            if (sector < 0 || behind || !shown[(size_t)sector]) continue;
            const dg::FloorCell cell = cells[(size_t)sector];
            if (cell.flat < 0) continue;
            const int tx = (int)std::floor(mx) & 63, ty = (int)std::floor(my) & 63;
            const uint8_t texel = sc.flat_pool[(size_t)cell.flat * 4096 + (size_t)ty * 64 + (size_t)tx];
            for (int ch = 0; ch < 3; ch++) {
                const float col = (float)sc.palette[3 * texel + ch] * cell.factor;
                px[ch] = (uint8_t)(col >= 255.0f ? 255 : col <= 0.0f ? 0 : (int)col);
            }
        }
    return 0;
}

// Part 2: dg_floor_map_tiles as a host loop.
static int phases_frame(const dg::Scene &sc, const Case &c, const dg_view &v, const uint32_t *mask, const std::vector<dg::FloorCell> &cells, const dg::FloorTables &T,
                        const dg::FloorHostTables &t, std::vector<uint8_t> &got) {
    const int W = c.W, H = c.H;
    std::vector<dg::EgoLine> lines;
    std::vector<uint32_t> words;
    dg::ego_line_table(sc, lines, words);
    const dg::EgoView ev = dg::ego_view(v);
    const bool rotate = (c.params.flags & DG_EGO_ROTATE) != 0;
    const float inv = 1.0f / c.params.scale;
    dg::MapSeg arrow[3] = {};
    if (c.params.flags & DG_EGO_ARROW) {
        dg_map_line l[3];
        std::string err;
        CHECK(dg::ego_arrow_lines(W, H, v, c.params, l, err) == DG_OK);
        for (int k = 0; k < 3; k++) arrow[k] = dg::map_seg_make(l[k].x0, l[k].y0, l[k].x1, l[k].y1, l[k].rgb, W, H);
    }
    std::vector<uint32_t> seen;
    if (mask) { seen.resize(dg::floor_seen_words(sc)); dg::floor_seen_row(sc, t, mask, seen.data()); }
    const uint32_t band_rows = dg::ego_band_rows((uint32_t)W), px_form = dg::ego_store_px((uint32_t)W, (uint32_t)H, 0);
    CHECK(dg::ego_bands((uint32_t)W, (uint32_t)H) == ((uint32_t)H + band_rows - 1) / band_rows);
    for (int row0 = 0; row0 < H; row0 += (int)band_rows) {
        const int rows = std::min((int)band_rows, H - row0);
        const uint32_t px = (uint32_t)rows * (uint32_t)W;
        CHECK(px <= (W > (int)dg::EGO_TILE_PX ? dg::EGO_WIDE_TILE_PX : dg::EGO_TILE_PX) && px % px_form == 0);
        std::vector<uint32_t> tile(px, 0u);                // exactly the band: an index outside it is the sanitizer's to report
        for (size_t l = 0; l < lines.size(); l++) {
            if (!(words[l] & dg::EGO_DRAWN) || (mask && !((mask[l >> 5] >> (l & 31u)) & 1u))) continue;
            const dg::MapSeg sg = dg::ego_band_seg(lines[l], words[l] & ~dg::EGO_DRAWN, ev, c.params.scale, rotate, W, H, row0, rows);
            for (int32_t k = 0; k < sg.count; k++) {
                int32_t x, y;
                dg::map_seg_point(sg, (int64_t)sg.first + k, x, y);
                CHECK(x >= 0 && x < W && y >= 0 && y < rows);
                uint32_t &w = tile[(size_t)y * (size_t)W + (size_t)x];
                w = std::max(w, sg.rgb);
            }
        }
        if (c.params.flags & DG_EGO_ARROW)
            for (const dg::MapSeg &a : arrow)
                for (int32_t k = 0; k < a.count; k++) {
                    int32_t x, y;
                    dg::map_seg_point(a, (int64_t)a.first + k, x, y);
                    y -= row0;
                    if (x >= 0 && x < W && y >= 0 && y < rows) tile[(size_t)y * (size_t)W + (size_t)x] = std::max(tile[(size_t)y * (size_t)W + (size_t)x], dg::EGO_ARROW_VALUE);
                }
        for (uint32_t j = 0; j < px; j++) {                // the floor phase
            if (tile[j] != 0u) continue;
            const uint32_t y = j / (uint32_t)W, x = j - y * (uint32_t)W;
            tile[j] = dg::floor_pixel(T, cells.data(), mask ? seen.data() : nullptr, (int32_t)x, row0 + (int32_t)y, W, H, ev, inv, rotate);
            CHECK(tile[j] == 0u || (tile[j] & dg::FLOOR_VALUE));
        }
        uint8_t *const out = got.data() + (size_t)3 * (size_t)row0 * (size_t)W;
        for (uint32_t j = 0; j < px / px_form; j++) {
            if (px_form == 1) {
                const uint32_t rgb = dg::floor_value_rgb(tile[j]);
                out[3 * j] = (uint8_t)rgb; out[3 * j + 1] = (uint8_t)(rgb >> 8); out[3 * j + 2] = (uint8_t)(rgb >> 16);
            } else {
                for (uint32_t g = 0; g < px_form / 4; g++) {
                    const uint32_t *w = &tile[(size_t)px_form * j + 4 * g];
                    uint32_t o[3];
                    dg::ego_pack4_rgb(dg::floor_value_rgb(w[0]), dg::floor_value_rgb(w[1]), dg::floor_value_rgb(w[2]), dg::floor_value_rgb(w[3]), o[0], o[1], o[2]);
                    for (int k = 0; k < 3; k++)
                        for (int b = 0; b < 4; b++) out[(size_t)3 * px_form * j + 12 * g + 4 * k + b] = (uint8_t)(o[k] >> (8 * b));       // little-endian stores
                }
            }
        }
    }
    return 0;
}

// Part 4: one pixel of a table set by a literal descent that checks no index (for sets all of whose indices are in range).
static uint32_t literal_table_pixel(const dg::FloorTables &T, const dg::FloorCell *row, const floor_tables_test::TestView &t, int X, int Y) {
    const float inv = 1.0f / t.scale;
    const float r = ((float)(X - t.W / 2) + 0.5f) * inv, f = ((float)(t.H / 2 - Y) - 0.5f) * inv;
    const float dx = t.rotate ? r * t.v.sin_a + f * t.v.cos_a : r, dy = t.rotate ? f * t.v.sin_a - r * t.v.cos_a : f;
    const float mx = t.v.x + dx, my = t.v.y + dy;
    int32_t c = (int32_t)T.n_nodes - 1;
    while (c >= 0) {
        const dg::WalkNode &n = T.nodes[c];
        const float v2x = n.x + n.dx, v2y = n.y + n.dy;
        const float ax = mx - n.x, ay = my - n.y, bx = v2x - n.x, by = v2y - n.y;
        c = ax * by - ay * bx <= 0.0f ? n.child[1] : n.child[0];
    }
    const dg::FloorLeaf &l = T.leaves[~c];
    if (l.sector < 0) return 0u;
    for (uint32_t k = 0; k < l.count; k++) {
        const dg::FloorSeg &g = T.segs[l.first + k];
        const float ax = mx - g.v1x, ay = my - g.v1y, bx = g.v2x - g.v1x, by = g.v2y - g.v1y;
        if (ax * by - ay * bx < 0.0f) return 0u;
    }
    const dg::FloorCell cell = row[l.sector];
    if (cell.flat < 0) return 0u;
    const int tx = (int)std::floor(mx) & 63, ty = (int)std::floor(my) & 63;
    const uint32_t pal = T.palette[T.flats[(size_t)cell.flat * 4096 + (size_t)ty * 64 + (size_t)tx]];
    uint32_t rgb = 0;
    for (int ch = 0; ch < 3; ch++) {
        const float col = (float)((pal >> (8 * ch)) & 255u) * cell.factor;
        rgb |= (uint32_t)(col >= 255.0f ? 255 : col <= 0.0f ? 0 : (int)col) << (8 * ch);
    }
    return rgb;
}

static int table_sets(uint64_t &lit_all) {
    using namespace floor_tables_test;
    const std::vector<TableSet> sets = all_sets();
    CHECK(sets.size() == 15);
    for (const TableSet &s : sets) {
        Exact e;
        exact(s, e);
        const std::vector<dg::FloorCell> row(s.row.begin(), s.row.begin() + s.n_sectors);       // exactly the frame's row
        uint64_t lit = 0, px = 0;
        for (const TestView &t : views_of(s)) {
            std::vector<uint8_t> got((size_t)3 * (size_t)t.W * (size_t)t.H);
            lit += rule_frame(e.T, row.data(), t, got.data());
            px += (uint64_t)t.W * (uint64_t)t.H;
            if (s.expect == TableSet::B_DARK) continue;     // (an index out of range: the literal descent is not defined there)
            for (int Y = 0; Y < t.H; Y++)
                for (int X = 0; X < t.W; X++) {
                    const uint8_t *const q = &got[3 * ((size_t)Y * (size_t)t.W + (size_t)X)];
                    CHECK(literal_table_pixel(e.T, row.data(), t, X, Y) == ((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16));
                }
        }
        if (!meets(s, lit, px)) { std::printf("floor_map_host_main: %s: %llu of %llu pixels lit\n", s.name.c_str(), (unsigned long long)lit, (unsigned long long)px); return 1; }
        lit_all += lit;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::printf("usage: floor_map_host_main WAD PATH.f32 MAP\n"); return 2; }
    std::ifstream wf(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(wf)), std::istreambuf_iterator<char>());
    std::ifstream pf(argv[2], std::ios::binary);
    std::vector<char> praw((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
    std::vector<float> path(praw.size() / 4);
    std::memcpy(path.data(), praw.data(), path.size() * 4);
    CHECK(!wad.empty() && path.size() >= 8 * 1000);
    dg_scene *s = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[3], &s) == DG_OK);
    const dg::Scene &sc = *s->sc;
    dg::FloorHostTables t;
    dg::floor_tables(sc, t);
    uint32_t pal[256];
    dg::floor_palette(sc, pal);
    const dg::FloorTables T = dg::floor_tables_host(sc, t, pal);

    const int sizes[4][2] = {{5, 3}, {131, 67}, {1, 1}, {8200, 2}};
    const float scales[3] = {0.05f, 1.0f, 16.0f};
    std::vector<Case> cases;
    int k = 0;
    for (const auto &sz : sizes)
        for (float scale : scales)
            for (uint32_t rot = 0; rot < 2; rot++, k++) {
                const float *r = &path[(size_t)8 * (size_t)((k * 97) % 1000)];
                dg_view v{};
                v.x = r[0]; v.y = r[1]; v.angle = r[2]; v.timestamp = 0.4f * (float)k;
                if (k % 2) { v.cos_a = r[3]; v.sin_a = r[4]; v.cos_na = r[5]; v.sin_na = r[6]; v.trig_valid = 1; }
                cases.push_back(Case{sz[0], sz[1], v, dg_ego_map{scale, rot | ((k % 3) ? (uint32_t)DG_EGO_ARROW : 0u)}, k % 3, k % 4 == 1});
            }
    uint64_t floor_px = 0, black_px = 0;
    dg::FloorRowScratch scratch;
    for (const Case &c : cases) {
        std::vector<uint32_t> mask((size_t)dg_seen_words(s), 0u);
        if (c.mask == 1) for (uint32_t &w : mask) w = rng32();
        const uint32_t *const mp = c.mask ? mask.data() : nullptr;
        Inputs in;
        inputs_of(sc, c, in);
        dg_view v = c.view;
        dg::fill_view_trig(v);
        std::vector<dg::FloorCell> cells(sc.sectors.size());
        std::string err;
        CHECK(dg::floor_view_cells(sc, &sc.fx.light, v, c.entries ? &in.state : nullptr, c.entries ? &in.surfaces : nullptr, scratch, cells.data(), err) == DG_OK);
        const size_t bytes = (size_t)3 * (size_t)c.W * (size_t)c.H;
        std::vector<uint8_t> want(bytes, 0), got(bytes, 0x5a);
        if (literal_frame(sc, c, v, mp, cells, want) || phases_frame(sc, c, v, mp, cells, T, t, got)) return 1;
        CHECK(got == want);
        if (c.W >= 16 && c.H >= 16) {
            std::vector<uint8_t> api(bytes, 0x5a);
            CHECK(dg_floor_map_host(s, c.W, c.H, &c.view, &c.params, mp, c.entries ? &in.state : nullptr, c.entries ? &in.surfaces : nullptr, api.data()) == DG_OK);
            CHECK(api == want);
        }
        for (size_t i = 0; i < bytes; i += 3) (want[i] | want[i + 1] | want[i + 2] ? floor_px : black_px)++;
    }
    CHECK(floor_px > 10000 && black_px > 1000);

    // what is refused, with no buffer touched
    const dg_view v0{};
    const dg_ego_map bad{0.0f, 0}, good{1.0f, 0};
    uint8_t one = 7;
    CHECK(dg_floor_map_host(s, 64, 40, &v0, &bad, nullptr, nullptr, nullptr, &one) == DG_ERR_INVALID && one == 7);
    CHECK(dg_floor_map_host(s, 15, 40, &v0, &good, nullptr, nullptr, nullptr, &one) == DG_ERR_INVALID && one == 7);
    const dg_sector_light far_light{(int32_t)sc.sectors.size(), 100};
    const dg_view_state st{&far_light, 1u, nullptr, 0u};
    CHECK(dg_floor_map_host(s, 64, 40, &v0, &good, nullptr, &st, nullptr, &one) == DG_ERR_INVALID && one == 7);
    const dg_sector_flats far_flat{0, 0x0fffffff, 0};
    const dg_view_surfaces sf{nullptr, 0u, &far_flat, 1u};
    CHECK(dg_floor_map_host(s, 64, 40, &v0, &good, nullptr, nullptr, &sf, &one) == DG_ERR_INVALID && one == 7);
    dg_scene_free(s);
    uint64_t table_px = 0;
    if (table_sets(table_px)) return 1;
    CHECK(table_px > 50000);
    std::printf("floor_map_host_main: ok (%llu lit pixels, %llu black, %llu lit on the table sets)\n", (unsigned long long)floor_px, (unsigned long long)black_px,
                (unsigned long long)table_px);
    return 0;
}
