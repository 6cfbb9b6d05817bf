// tests/map_things/map_things_host_main.cpp WAD MAP — the host side of the map-object markers on the map frames as a stand-alone
// program, for a sanitizer build (tests/test_map_things_host.py builds it with -fsanitize=address,undefined together with the library's
// host sources and runs it).  Three parts:
//   1. dg_map_thing_lines, dg_ego_map_things_host and dg_floor_map_things_host through the C-ABI, with buffers of exactly the sizes the
//      contract names;
//   2. the band kernels' phases as a host loop over the shared inline functions — the linedefs (ego_band_seg), the things phase
//      (thing_band_seg over items (object, edge) in chunks of EGO_CHUNK, from the frame's shown bits and sorted entries), the arrow, and
//      the resolve through the marker table — for EVERY band height from 1 to H, against dg_ego_map_things_host, byte for byte;
//   3. the same with the floor phase behind the things phase at the kernel's own band rows, against dg_floor_map_things_host.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/map_things_host.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("map_things_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

struct Case {
    int W, H;
    dg_view view;
    dg_ego_map params;
    bool masked;
    std::vector<dg_mobj_pose> poses;
    std::vector<dg_mobj_state> states;
};

// What a *_things submission ships for one frame, built as context.cpp builds it.
struct Frame {
    std::vector<dg::ThingMarker> tm;
    std::vector<dg::ThingPlace> tp;
    std::vector<uint32_t> row;
    std::vector<dg::ThingEntry> entries;
};

static int build_frame(const dg_scene *s, const Case &c, Frame &f) {
    const dg::Scene &sc = *s->sc;
    dg::thing_tables(sc, sc.markers, f.tm, f.tp);
    f.row.assign(dg::thing_shown_words((uint32_t)sc.mobjs.size()), 0u);
    f.entries.clear();
    dg::ThingViewScratch scratch;
    std::string err;
    dg_view v = c.view;
    dg::fill_view_trig(v);
    const dg_view_state st{nullptr, 0u, c.states.data(), (uint32_t)c.states.size()};
    const dg_view_poses ps{c.poses.data(), (uint32_t)c.poses.size()};
    CHECK(dg::thing_view_rows(sc, sc.markers, &sc.fx.mobj, v, &st, &ps, scratch, f.row.data(), f.entries, err) == DG_OK);
    for (size_t k = 1; k < f.entries.size(); k++) CHECK(f.entries[k - 1].mobj < f.entries[k].mobj);      // sorted, one per object
    return 0;
}

// The phases of one band into `tile` (exactly the band: an index outside it is the sanitizer's to report).
static int band_tile(const dg::Scene &sc, const Case &c, const std::vector<uint32_t> &mask, const Frame &f, const dg::EgoView &ev, const dg::MapSeg *arrow, int row0,
                     int rows, std::vector<uint32_t> &tile, uint64_t &thing_steps) {
    const int W = c.W, H = c.H;
    const bool rotate = (c.params.flags & DG_EGO_ROTATE) != 0;
    std::vector<dg::EgoLine> lines;
    std::vector<uint32_t> words;
    dg::ego_line_table(sc, lines, words);
    tile.assign((size_t)rows * (size_t)W, 0u);
    auto walk = [&](const std::vector<dg::MapSeg> &list, uint64_t *steps) {
        for (size_t e = list.size(); e-- > 0;)             // (backwards: the order must not matter)
            for (int32_t k = 0; k < list[e].count; k++) {
                int32_t x, y;
                dg::map_seg_point(list[e], (int64_t)list[e].first + k, x, y);
                if (x < 0 || x >= W || y < 0 || y >= rows) return 1;
                uint32_t &t = tile[(size_t)y * (size_t)W + (size_t)x];
                t = std::max(t, list[e].rgb);
                if (steps) ++*steps;
            }
        return 0;
    };
    for (size_t base = 0; base < lines.size(); base += dg::EGO_CHUNK) {
        std::vector<dg::MapSeg> list;
        for (size_t l = base; l < std::min(lines.size(), base + dg::EGO_CHUNK); l++) {
            if (!(words[l] & dg::EGO_DRAWN) || (c.masked && !((mask[l >> 5] >> (l & 31u)) & 1u))) continue;
            const dg::MapSeg sg = dg::ego_band_seg(lines[l], words[l] & ~dg::EGO_DRAWN, ev, c.params.scale, rotate, W, H, row0, rows);
            if (sg.count > 0) list.push_back(sg);
        }
        CHECK(list.size() <= dg::EGO_CHUNK && walk(list, nullptr) == 0);
    }
    const uint32_t n_items = (uint32_t)f.tm.size() * dg::THING_EDGES;
    for (uint32_t base = 0; base < n_items; base += dg::EGO_CHUNK) {
        std::vector<dg::MapSeg> list;
        for (uint32_t item = base; item < std::min(n_items, base + dg::EGO_CHUNK); item++) {
            const uint32_t mobj = item / dg::THING_EDGES, edge = item - mobj * dg::THING_EDGES;
            const dg::MapSeg sg = dg::thing_band_seg(mobj, edge, f.row.data(), f.tm.data(), f.entries.data(), (uint32_t)f.entries.size(), f.tp.data(), ev,
                                                     c.params.scale, rotate, W, H, row0, rows);
            if (sg.count > 0) {
                CHECK(dg::thing_is_value(sg.rgb) && dg::thing_value_object(sg.rgb) == mobj && sg.rgb > 131071u && sg.rgb < dg::EGO_ARROW_VALUE);
                list.push_back(sg);
            }
        }
        CHECK(list.size() <= dg::EGO_CHUNK && walk(list, &thing_steps) == 0);
    }
    if (c.params.flags & DG_EGO_ARROW)
        for (int a = 0; a < 3; a++) {
            int32_t lo, hi;
            dg::ego_seg_rows(arrow[a], lo, hi);
            if (arrow[a].count <= 0 || hi < row0 || lo >= row0 + rows) continue;
            for (int32_t k = 0; k < arrow[a].count; k++) {
                int32_t x, y;
                dg::map_seg_point(arrow[a], (int64_t)arrow[a].first + k, x, y);
                y -= row0;
                if (x >= 0 && x < W && y >= 0 && y < rows) tile[(size_t)y * (size_t)W + (size_t)x] = std::max(tile[(size_t)y * (size_t)W + (size_t)x], dg::EGO_ARROW_VALUE);
            }
        }
    return 0;
}

static int check_case(const dg_scene *s, const Case &c, uint64_t &thing_steps, uint64_t &marker_px) {
    const dg::Scene &sc = *s->sc;
    const int W = c.W, H = c.H;
    const size_t bytes = (size_t)3 * (size_t)W * (size_t)H;
    std::vector<uint32_t> mask((size_t)dg_seen_words(s));
    for (size_t k = 0; k < mask.size(); k++) mask[k] = 0x9e3779b9u * (uint32_t)(k + 7) | 0x10101u;
    const uint32_t *const mp = c.masked ? mask.data() : nullptr;
    const dg_view_state st{nullptr, 0u, c.states.data(), (uint32_t)c.states.size()};
    const dg_view_poses ps{c.poses.data(), (uint32_t)c.poses.size()};
    // part 1
    const int n = dg_map_thing_lines(s, W, H, &c.view, &c.params, &st, &ps, nullptr, 0);
    CHECK(n >= 0);
    std::vector<dg_map_line> tl((size_t)n);
    CHECK(dg_map_thing_lines(s, W, H, &c.view, &c.params, &st, &ps, tl.data(), n) == n);
    std::vector<uint8_t> want(bytes, 0x5a), want_floor(bytes, 0x5a), got(bytes, 0x5a);
    CHECK(dg_ego_map_things_host(s, W, H, &c.view, &c.params, mp, &st, &ps, want.data()) == DG_OK);
    CHECK(dg_floor_map_things_host(s, W, H, &c.view, &c.params, mp, &st, nullptr, &ps, want_floor.data()) == DG_OK);
    // parts 2 and 3
    Frame f;
    if (build_frame(s, c, f)) return 1;
    dg_view v = c.view;
    dg::fill_view_trig(v);
    const dg::EgoView ev = dg::ego_view(v);
    dg::MapSeg arrow[3] = {};
    if (c.params.flags & DG_EGO_ARROW) {
        dg_map_line l[3];
        std::string err;
        CHECK(dg::ego_arrow_lines(W, H, v, c.params, l, err) == DG_OK);
        for (int k = 0; k < 3; k++) arrow[k] = dg::map_seg_make(l[k].x0, l[k].y0, l[k].x1, l[k].y1, l[k].rgb, W, H);
    }
    const auto rgb = [&](uint32_t w) { return dg::thing_is_value(w) ? dg::thing_value_rgb(w, f.tm.data(), (uint32_t)f.tm.size()) : dg::floor_value_rgb(w); };
    std::vector<uint32_t> tile;
    for (int band_rows = 1; band_rows <= H; band_rows++) {
        std::fill(got.begin(), got.end(), 0x5a);
        for (int row0 = 0; row0 < H; row0 += band_rows) {
            const int rows = std::min(band_rows, H - row0);
            if (band_tile(sc, c, mask, f, ev, arrow, row0, rows, tile, thing_steps)) return 1;
            for (size_t j = 0; j < tile.size(); j++) {
                const uint32_t col = rgb(tile[j]);
                uint8_t *const o = got.data() + 3 * ((size_t)row0 * (size_t)W + j);
                o[0] = (uint8_t)col; o[1] = (uint8_t)(col >> 8); o[2] = (uint8_t)(col >> 16);
                marker_px += dg::thing_is_value(tile[j]);
            }
        }
        CHECK(got == want);
    }
    // the floor phase behind the things phase, at the kernel's own rows
    dg::FloorFrameHost F;
    std::string err;
    CHECK(dg::floor_frame_prepare(sc, &sc.fx.light, v, mp, &st, nullptr, F, err) == DG_OK);
    const dg::FloorTables T = dg::floor_tables_host(sc, F.t, F.pal);
    const float inv = 1.0f / c.params.scale;
    const int band_rows = (int)dg::ego_band_rows((uint32_t)W);
    std::fill(got.begin(), got.end(), 0x5a);
    for (int row0 = 0; row0 < H; row0 += band_rows) {
        const int rows = std::min(band_rows, H - row0);
        if (band_tile(sc, c, mask, f, ev, arrow, row0, rows, tile, thing_steps)) return 1;
        for (size_t j = 0; j < tile.size(); j++) {
            if (tile[j] == 0u) tile[j] = dg::floor_pixel(T, F.row.data(), mp ? F.seen.data() : nullptr, (int32_t)(j % (size_t)W), row0 + (int32_t)(j / (size_t)W), W, H, ev, inv,
                                                        (c.params.flags & DG_EGO_ROTATE) != 0);
            const uint32_t col = rgb(tile[j]);
            uint8_t *const o = got.data() + 3 * ((size_t)row0 * (size_t)W + j);
            o[0] = (uint8_t)col; o[1] = (uint8_t)(col >> 8); o[2] = (uint8_t)(col >> 16);
        }
    }
    CHECK(got == want_floor);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: map_things_host_main WAD MAP\n"); return 2; }
    std::ifstream wf(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(wf)), std::istreambuf_iterator<char>());
    CHECK(!wad.empty());
    dg_scene *s = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[2], &s) == DG_OK);
    const int n = dg_scene_mobj_count(s);
    CHECK(n >= 8);
    std::vector<dg_map_marker> markers((size_t)n);
    for (int i = 0; i < n; i++) markers[(size_t)i] = dg_map_marker{i % 5 == 4 ? 0 : 8 + 24 * (i % 4), 0x80u | ((uint32_t)(37 * i + 80) & 255u) << 16, i % 7 == 3 ? 0u : 1u + (uint32_t)(i % 3)};
    markers[1].rgb = 0u;                                   // a black marker: its pixels are no floor pixels
    CHECK(dg_scene_set_map_markers(s, markers.data(), n) == DG_OK);
    std::vector<dg_mobj_placed> placed((size_t)n);
    CHECK(dg_scene_mobj_poses(s, placed.data(), n) == DG_OK);

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<Case> cases;
    const int sizes[3][2] = {{64, 48}, {44, 41}, {16, 16}};
    const float scales[4] = {0.05f, 0.25f, 1.0f, 4.0f};
    int k = 0;
    for (const auto &sz : sizes)
        for (float scale : scales)
            for (uint32_t rot = 0; rot < 2; rot++, k++) {
                const dg_mobj_placed &at = placed[(size_t)((k * 5) % n)];
                dg_view v{};
                v.x = at.x + 3.5f * (float)(k % 3); v.y = at.y - 2.25f * (float)(k % 4); v.angle = 0.37f * (float)k;
                Case c{sz[0], sz[1], v, dg_ego_map{scale, rot | ((k % 3) ? (uint32_t)DG_EGO_ARROW : 0u)}, k % 4 == 1, {}, {}};
                const int m = (k * 5) % n, m2 = (k * 5 + 1) % n;
                if (k % 2) c.poses = {dg_mobj_pose{m2, at.x + 9.0f, at.y + 4.0f, 1.0f}, dg_mobj_pose{m, at.x - 20.0f, at.y, 0.5f}, dg_mobj_pose{m2, at.x + 5.5f, at.y - 7.25f, nan},
                                      dg_mobj_pose{(m + 2) % n, nan, 0.0f, 0.0f}, dg_mobj_pose{(m + 3) % n, 32768.5f, at.y, 0.0f}, dg_mobj_pose{(m + 4) % n, at.x, inf, 0.0f}};
                if (k % 3 == 2) c.states = {dg_mobj_state{m, -1, 0, 0}, dg_mobj_state{m2, -1, 0, 0}, dg_mobj_state{m2, 0, 1, 0}};
                cases.push_back(c);
            }
    uint64_t thing_steps = 0, marker_px = 0;
    for (const Case &c : cases)
        if (check_case(s, c, thing_steps, marker_px)) return 1;
    CHECK(thing_steps > 10000 && marker_px > 10000);

    // what is refused, with no buffer touched
    const dg_view v0{};
    const dg_ego_map bad{0.0f, 0}, good{1.0f, 0};
    uint8_t one = 7;
    CHECK(dg_ego_map_things_host(s, 64, 48, &v0, &bad, nullptr, nullptr, nullptr, &one) == DG_ERR_INVALID && one == 7);
    CHECK(dg_floor_map_things_host(s, 15, 48, &v0, &good, nullptr, nullptr, nullptr, nullptr, &one) == DG_ERR_INVALID && one == 7);
    const dg_mobj_pose out_of_range{n, 0.0f, 0.0f, 0.0f};
    const dg_view_poses bad_poses{&out_of_range, 1u};
    CHECK(dg_ego_map_things_host(s, 64, 48, &v0, &good, nullptr, nullptr, &bad_poses, &one) == DG_ERR_INVALID && one == 7);
    CHECK(dg_map_thing_lines(s, 64, 48, &v0, &good, nullptr, &bad_poses, nullptr, 0) == DG_ERR_INVALID);
    CHECK(dg_scene_set_map_markers(s, nullptr, 0) == DG_OK && dg_map_thing_lines(s, 64, 48, &v0, &good, nullptr, nullptr, nullptr, 0) == 0);
    dg_scene_free(s);
    std::printf("map_things_host_main: ok (%llu marker steps, %llu marker pixels)\n", (unsigned long long)thing_steps, (unsigned long long)marker_px);
    return 0;
}
