// tests/bundle/bundle_host_main.cpp — the host side of a bundle submission as a stand-alone program, for a sanitizer build
// (tests/test_bundle_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
//   usage: bundle_host_main <wad file> <camera path .f32> <map name>
// Through the C-ABI alone: dg_bundle_lists_host on a frame built by hand here (a floor, a sky, an opaque wall, two masked textures owned
// by map objects, a column of 20 records, columns outside the frame) and on dg_build_lists_owners output for a few path frames, at several
// sizes; dg_bundle_layout for every `what`.  It checks what it gets: every output must equal dg_depth_lists_host's and
// dg_label_lists_host's, with any output left out, and a refused call writes nothing.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/doomgpu.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("bundle_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

struct Outputs {
    std::vector<int16_t> dist;
    std::vector<uint8_t> kind, cls;
    std::vector<uint16_t> id;
    std::vector<dg_label_box> boxes;
    Outputs(size_t px, size_t n_boxes) : dist(px, 77), kind(px, 77), cls(px, 77), id(px, 77), boxes(n_boxes) { std::memset(boxes.data(), 0x4d, n_boxes * sizeof(dg_label_box)); }
};

static bool same_boxes(const std::vector<dg_label_box> &a, const std::vector<dg_label_box> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].pixels != b[i].pixels || a[i].x0 != b[i].x0 || a[i].y0 != b[i].y0 || a[i].x1 != b[i].x1 || a[i].y1 != b[i].y1) return false;
    return true;
}

// n frames: the bundle's outputs against the two separate host entries, all at once and with each output left out in turn.
static int compare(const dg_scene *sc, int W, int H, const dg_frame_lists *frames, const uint32_t *const *owners, int n, int n_mobjs, uint64_t &mobj_pixels, uint64_t &sky_pixels) {
    const size_t px = (size_t)n * (size_t)W * (size_t)H, nb = (size_t)n * (size_t)n_mobjs;
    Outputs want(px, nb);
    CHECK(dg_depth_lists_host(sc, W, H, frames, n, want.dist.data(), want.kind.data()) == DG_OK);
    CHECK(dg_label_lists_host(sc, W, H, frames, owners, n, want.id.data(), want.cls.data(), want.boxes.data()) == DG_OK);
    for (int skip = -1; skip < 5; skip++) {
        Outputs got(px, nb);
        CHECK(dg_bundle_lists_host(sc, W, H, frames, owners, n, skip == 0 ? nullptr : got.dist.data(), skip == 1 ? nullptr : got.kind.data(),
                                   skip == 2 ? nullptr : got.id.data(), skip == 3 ? nullptr : got.cls.data(), skip == 4 ? nullptr : got.boxes.data()) == DG_OK);
        const Outputs untouched(px, nb);
        CHECK(got.dist == (skip == 0 ? untouched.dist : want.dist));
        CHECK(got.kind == (skip == 1 ? untouched.kind : want.kind));
        CHECK(got.id == (skip == 2 ? untouched.id : want.id));
        CHECK(got.cls == (skip == 3 ? untouched.cls : want.cls));
        CHECK(same_boxes(got.boxes, skip == 4 ? untouched.boxes : want.boxes));
    }
    // the depth planes alone need no owners
    Outputs depth_only(px, nb);
    CHECK(dg_bundle_lists_host(sc, W, H, frames, nullptr, n, depth_only.dist.data(), depth_only.kind.data(), nullptr, nullptr, nullptr) == DG_OK);
    CHECK(depth_only.dist == want.dist && depth_only.kind == want.kind);
    for (const dg_label_box &b : want.boxes) mobj_pixels += b.pixels;
    for (uint8_t k : want.kind) sky_pixels += k == DG_KIND_SKY;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), {});
    std::ifstream pf(argv[2], std::ios::binary);
    std::vector<float> path(8000);
    pf.read((char *)path.data(), 32000);
    dg_scene *sc = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[3], &sc) == DG_OK);
    const int n_mobjs = dg_scene_mobj_count(sc);
    CHECK(n_mobjs > 2);
    uint64_t mobj_pixels = 0, sky_pixels = 0, frames = 0;

    // ---- the frame built by hand, at three sizes ---------------------------------------------------------------------------------------
    const int brick = dg_scene_texture_id(sc, "BRICK1"), grate = dg_scene_texture_id(sc, "GRATE1"), holey = dg_scene_texture_id(sc, "HOLEY1");
    const int floor1 = dg_scene_flat_id(sc, "FLOOR1", 0.0f), sky = dg_scene_flat_id(sc, "F_SKY1", 0.0f);
    CHECK(brick >= 0 && grate >= 0 && holey >= 0 && floor1 >= 0 && sky != floor1);
    const int sizes[][2] = {{64, 40}, {131, 67}, {5, 9}};
    for (auto &s : sizes) {
        const int W = s[0], H = s[1], m = H / 2;
        std::vector<dg_bitmap_column> cols;
        std::vector<dg_bitmap_render> renders;
        auto wall = [&](int bitmap, int light, float x0, float y0, float x1, float y1, int sx, int ex, size_t first) {
            renders.push_back(dg_bitmap_render{bitmap, (int16_t)light, 3, -5, 0, x0, y0, x1, y1, 1.5f, sx, ex, -41.0f, 87.0f, (uint32_t)first, (uint32_t)(cols.size() - first)});
        };
        size_t first = cols.size();                                                   // 0: an opaque wall over the middle third, one column left of the frame
        cols.push_back(dg_bitmap_column{(int16_t)-2, 0, (int16_t)(H - 1), (int16_t)(H + 3), (int16_t)-4});
        for (int x = W / 3; x < 2 * W / 3 + 1 && x < W; x++) cols.push_back(dg_bitmap_column{(int16_t)x, 2, (int16_t)(H - 3 > 2 ? H - 3 : 2), (int16_t)(H + 3), (int16_t)-4});
        wall(brick, 160, 100.0f, -30.0f, 180.0f, 50.0f, W / 3, 2 * W / 3, first);
        first = cols.size();                                                          // 1: a masked texture in one- and two-row columns over everything
        for (int x = 0; x < W; x++) cols.push_back(dg_bitmap_column{(int16_t)x, (int16_t)m, (int16_t)(m + x % 2 < H ? m + x % 2 : H - 1), 45, -6});
        wall(grate, 255, 40.0f, -20.0f, 44.0f, 20.0f, 0, W - 1, first);
        first = cols.size();                                                          // 2: a holey one over the upper rows, two columns right of the frame
        for (int x = 0; x < W + 2; x++) cols.push_back(dg_bitmap_column{(int16_t)x, 0, (int16_t)(m > 2 ? m - 2 : 0), 36, 4});
        wall(holey, 208, 80.0f, -40.0f, 120.0f, 40.0f, 0, W + 1, first);
        for (int k = 0; k < 20; k++) {                                                // 3..22: twenty records on column 1 (column 0 where there is no other)
            first = cols.size();
            const int x = W > 1 ? 1 : 0;
            cols.push_back(dg_bitmap_column{(int16_t)x, (int16_t)(k % H), (int16_t)((k % H) + 2 < H ? (k % H) + 2 : H - 1), (int16_t)(H + k), (int16_t)-k});
            wall(k % 2 ? holey : brick, 100 + k, 50.0f, 5.0f + (float)k, 70.0f, -5.0f, x, x, first);
        }
        std::vector<int16_t> tb;
        std::vector<dg_visplane> planes;
        planes.push_back(dg_visplane{floor1, 0, 200, 0, (int16_t)(W - 1), (uint32_t)(tb.size() / 2)});
        for (int x = 0; x < W; x++) { tb.push_back((int16_t)(m - 1 - x % 3 > 0 ? m - 1 - x % 3 : 0)); tb.push_back((int16_t)(H - 1)); }
        planes.push_back(dg_visplane{sky, 128, 255, 0, (int16_t)(W - 1), (uint32_t)(tb.size() / 2)});
        for (int x = 0; x < W; x++) { tb.push_back(0); tb.push_back((int16_t)(x % 4)); }
        std::vector<dg_draw_cmd> order = {{1, 0}, {0, 0}, {1, 1}, {0, 1}, {0, 2}};
        for (uint32_t k = 3; k < (uint32_t)renders.size(); k++) order.push_back(dg_draw_cmd{0, k});
        dg_frame_lists fl{};
        fl.view = dg_view{1000.3f, -740.8f, 0.7f, 0.0f, 0, 0, 0, 0, 0.0f, 0};
        fl.renders = renders.data(); fl.n_renders = (uint32_t)renders.size();
        fl.columns = cols.data(); fl.n_columns = (uint32_t)cols.size();
        fl.visplanes = planes.data(); fl.n_visplanes = (uint32_t)planes.size();
        fl.plane_tb = tb.data(); fl.n_plane_tb = (uint32_t)tb.size();
        fl.order = order.data(); fl.n_order = (uint32_t)order.size();
        std::vector<uint32_t> owners(renders.size()), other(renders.size());
        for (size_t i = 0; i < owners.size(); i++) {                                  // odd records are map objects, even ones wall segs
            owners[i] = i % 2 ? ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)((5 * i) % (size_t)n_mobjs) : ((uint32_t)DG_LABEL_WALL << 16) | (uint32_t)i;
            other[i] = ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)(n_mobjs - 1);
        }
        const dg_frame_lists two[2] = {fl, fl};
        const uint32_t *const own2[2] = {owners.data(), other.data()};
        if (compare(sc, W, H, two, own2, 2, n_mobjs, mobj_pixels, sky_pixels)) return 1;
        frames += 2;
        CHECK(sky_pixels > 0 && mobj_pixels > 0);                                     // the hand-built frame shows a sky and map objects
        // refused calls write nothing: labels without owners, a NULL owners[f], every bad tag in the second frame
        const size_t px = 2 * (size_t)W * (size_t)H;
        Outputs got(px, 2 * (size_t)n_mobjs);
        const Outputs untouched(px, 2 * (size_t)n_mobjs);
        CHECK(dg_bundle_lists_host(sc, W, H, two, nullptr, 2, got.dist.data(), got.kind.data(), got.id.data(), nullptr, nullptr) == DG_ERR_INVALID);
        const uint32_t *const on[2] = {owners.data(), nullptr};
        CHECK(dg_bundle_lists_host(sc, W, H, two, on, 2, got.dist.data(), got.kind.data(), nullptr, got.cls.data(), nullptr) == DG_ERR_INVALID);
        const uint32_t bad_tags[] = {0u, 3u << 16, ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)n_mobjs, ((uint32_t)DG_LABEL_WALL << 16) | 0xffffu, 0xffffffffu};
        for (uint32_t t : bad_tags) {
            std::vector<uint32_t> bad(owners);
            bad.back() = t;
            const uint32_t *const ob[2] = {owners.data(), bad.data()};
            CHECK(dg_bundle_lists_host(sc, W, H, two, ob, 2, got.dist.data(), got.kind.data(), got.id.data(), got.cls.data(), got.boxes.data()) == DG_ERR_INVALID);
            CHECK(std::strstr(dg_last_error(), "frame 1") != nullptr);
            CHECK(dg_bundle_lists_host(sc, W, H, two, ob, 2, got.dist.data(), got.kind.data(), nullptr, nullptr, nullptr) == DG_OK);   // (the tags are not read without a label output)
            got.dist = untouched.dist; got.kind = untouched.kind;
        }
        CHECK(got.dist == untouched.dist && got.kind == untouched.kind && got.id == untouched.id && got.cls == untouched.cls && same_boxes(got.boxes, untouched.boxes));
        CHECK(dg_bundle_lists_host(sc, W, H, two, own2, 0, got.dist.data(), got.kind.data(), got.id.data(), got.cls.data(), got.boxes.data()) == DG_OK && got.cls == untouched.cls);
        CHECK(dg_bundle_lists_host(sc, W, H, two, own2, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == DG_OK);
    }

    // ---- the library's own lists for a few path frames ---------------------------------------------------------------------------------
    const int path_sizes[][2] = {{160, 100}, {64, 200}};
    for (auto &s : path_sizes)
        for (int i = 0; i < 1000; i += 333) {
            const float *r = &path[(size_t)i * 8];
            const dg_view v{r[0], r[1], r[2], r[7], r[3], r[4], r[5], r[6], 0.0f, 1};
            dg_frame_lists fl;
            const uint32_t *owners = nullptr;
            CHECK(dg_build_lists_owners(sc, s[0], s[1], &v, &fl, &owners) == DG_OK);
            const uint32_t *const own1[1] = {owners};
            if (compare(sc, s[0], s[1], &fl, own1, 1, n_mobjs, mobj_pixels, sky_pixels)) return 1;
            frames++;
        }
    CHECK(mobj_pixels > 0);

    // ---- the layout -------------------------------------------------------------------------------------------------------------------
    for (uint32_t what = 1; what < 8; what++) {
        dg_bundle_offsets o;
        CHECK(dg_bundle_layout(5, 9, 3, what, &o) == DG_OK);
        CHECK(o.total > 0 && (!(what & DG_BUNDLE_DEPTH) || o.distance % 2 == 0) && (!(what & DG_BUNDLE_LABELS) || o.id % 2 == 0));   // (3nWH = 405 is odd)
        CHECK(((what & DG_BUNDLE_COLOUR) ? o.colour == 0 : o.colour == o.total) && ((what & DG_BUNDLE_DEPTH) ? o.kind < o.total : o.kind == o.total));
    }
    dg_bundle_offsets o;
    CHECK(dg_bundle_layout(5, 9, 3, 0, &o) == DG_ERR_INVALID && dg_bundle_layout(5, 9, 3, 8, &o) == DG_ERR_INVALID && dg_bundle_layout(5, 9, 3, 7, nullptr) == DG_ERR_INVALID);
    dg_scene_free(sc);
    std::printf("bundle_host_main: ok (%llu frames, %llu map-object pixels)\n", (unsigned long long)frames, (unsigned long long)mobj_pixels);
    return 0;
}
