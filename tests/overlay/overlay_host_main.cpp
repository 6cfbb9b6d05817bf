// tests/overlay/overlay_host_main.cpp — the host side of the screen pictures as a stand-alone program, for a sanitizer build
// (tests/test_overlay_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
//   overlay_host_main <wad> <map> <picture name>...
// Through the C-ABI: dg_overlay_host on a 5x3 and a 131x67 frame with items hanging over every edge and corner, and on a 1x1 frame, the
// frames in heap memory of exactly 3 W H n bytes (one byte outside is a report), each result compared with a painter's loop written here
// from the header's rule with plain divisions.  From overlay_core.h: ovl_div against `/` over its whole domain.  From overlay_plan.hpp:
// the rectangles of every such call are inside the frame, disjoint within a frame, and hold every pixel an item covers.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/overlay_plan.hpp"
#include "../../include/doomgpu.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("overlay_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Pic { int32_t handle, w, h, l, t; std::vector<int16_t> px; };   // px[y * w + x]: the palette index, or -1

// One 1x1 draw of the picture alone on a frame of its size shows its texels: two fills tell a texel from a hole.
static int read_picture(const dg_scene *s, const uint8_t *palette, Pic &p) {
    CHECK(dg_scene_picture_info(s, p.handle, &p.w, &p.h, &p.l, &p.t) == DG_OK);
    CHECK(p.w >= 1 && p.h >= 1);
    const size_t bytes = 3u * (size_t)p.w * (size_t)p.h;
    std::unique_ptr<uint8_t[]> a(new uint8_t[bytes]), b(new uint8_t[bytes]);
    std::memset(a.get(), 0x00, bytes); std::memset(b.get(), 0xff, bytes);
    const dg_screen_picture it{p.handle, 0, 0, 1, 1, 255, 0};
    const uint32_t first[2] = {0, 1};
    CHECK(dg_overlay_host(s, a.get(), p.w, p.h, 1, &it, first) == DG_OK);
    CHECK(dg_overlay_host(s, b.get(), p.w, p.h, 1, &it, first) == DG_OK);
    p.px.assign((size_t)p.w * p.h, -1);
    for (size_t i = 0; i < p.px.size(); i++) {
        if (std::memcmp(a.get() + 3 * i, b.get() + 3 * i, 3) != 0) continue;     // a hole: both fills show through
        for (int v = 0; v < 256 && p.px[i] < 0; v++)
            if (std::memcmp(palette + 3 * v, a.get() + 3 * i, 3) == 0) p.px[i] = (int16_t)v;
        CHECK(p.px[i] >= 0);
    }
    return 0;
}

static void paint(std::vector<uint8_t> &frames, int W, int H, int f, const dg_screen_picture &it, const Pic &p, const uint8_t *palette) {
    const int64_t sx = it.scale_x, sy = it.scale_y;
    const int64_t ox = it.x - ((it.flags & DG_PIC_OFFSETS) ? p.l * sx : 0), oy = it.y - ((it.flags & DG_PIC_OFFSETS) ? p.t * sy : 0);
    const float factor = (float)it.light_level / 255.0f;
    for (int64_t py = 0; py < H; py++)
        for (int64_t px = 0; px < W; px++) {
            if (px < ox || px >= ox + p.w * sx || py < oy || py >= oy + p.h * sy) continue;
            int64_t tx = (px - ox) / sx;
            const int64_t ty = (py - oy) / sy;
            if (it.flags & DG_PIC_MIRROR) tx = p.w - 1 - tx;
            const int16_t v = p.px[(size_t)(ty * p.w + tx)];
            if (v < 0) continue;
            for (int c = 0; c < 3; c++) frames[((size_t)f * H * W + (size_t)(py * W + px)) * 3 + c] = (uint8_t)((float)palette[3 * v + c] * factor);
        }
}

static int check_plan(const std::vector<Pic> &pics, int W, int H, int n, const std::vector<dg_screen_picture> &items, const std::vector<uint32_t> &first) {
    std::vector<dg::OvlPicture> table;
    for (const Pic &p : pics) table.push_back(dg::OvlPicture{p.w, p.h, p.l, p.t, 0u});
    CHECK(dg::overlay_check((int32_t)table.size(), W, H, n, items.data(), first.data()) == nullptr);
    dg::OvlPlan plan;
    dg::overlay_plan(table.data(), W, H, n, items.data(), first.data(), plan);
    std::vector<uint8_t> in_rect((size_t)n * W * H, 0);
    for (const dg::OvlRect &r : plan.rects) {
        CHECK((int)r.frame < n && r.x0 < r.x1 && r.y0 < r.y1 && r.x1 <= W && r.y1 <= H && r.item0 < r.item1 && r.item1 <= plan.items.size());
        const uint32_t tiles_y = (r.y1 - r.y0 + dg::OVL_TILE_H - 1u) / dg::OVL_TILE_H;
        CHECK(r.tiles_x == (r.x1 - r.x0 + dg::OVL_TILE_W - 1u) / dg::OVL_TILE_W && r.tiles >= 1 && r.tiles <= plan.max_tiles && plan.max_tiles <= dg::OVL_TILES_PER_RECT);
        CHECK(r.tile0 + r.tiles <= r.tiles_x * tiles_y);
        for (uint32_t t = r.tile0; t < r.tile0 + r.tiles; t++)
            for (uint32_t y = r.y0 + (t / r.tiles_x) * dg::OVL_TILE_H; y < r.y0 + (t / r.tiles_x + 1u) * dg::OVL_TILE_H && y < r.y1; y++)
                for (uint32_t x = r.x0 + (t % r.tiles_x) * dg::OVL_TILE_W; x < r.x0 + (t % r.tiles_x + 1u) * dg::OVL_TILE_W && x < r.x1; x++)
                    CHECK(in_rect[((size_t)r.frame * H + y) * W + x]++ == 0);               // once: the rectangles of a frame are disjoint
    }
    for (int f = 0; f < n; f++)
        for (uint32_t i = first[(size_t)f]; i < first[(size_t)f + 1]; i++) {
            dg::OvlItem o;
            if (!dg::ovl_resolve(items[i], table[(size_t)items[i].picture], W, H, o)) continue;
            CHECK(o.x0 >= 0 && o.y0 >= 0 && o.x1 <= W && o.y1 <= H && o.ox <= o.x0 && o.oy <= o.y0);
            for (int y = o.y0; y < o.y1; y++)
                for (int x = o.x0; x < o.x1; x++) CHECK(in_rect[((size_t)f * H + (size_t)y) * W + (size_t)x] == 1);
        }
    return 0;
}

static int run(const dg_scene *s, const std::vector<Pic> &pics, const uint8_t *palette, int W, int H, int n, const std::vector<dg_screen_picture> &items,
               const std::vector<uint32_t> &first, uint64_t &changed) {
    const size_t bytes = 3u * (size_t)W * (size_t)H * (size_t)n;
    std::unique_ptr<uint8_t[]> frames(new uint8_t[bytes]);                 // exactly the frames: a byte outside is a report
    std::vector<uint8_t> want(bytes);
    for (size_t i = 0; i < bytes; i++) want[i] = frames[i] = (uint8_t)rng();
    for (int f = 0; f < n; f++)
        for (uint32_t i = first[(size_t)f]; i < first[(size_t)f + 1]; i++) paint(want, W, H, f, items[i], pics[(size_t)items[i].picture], palette);
    CHECK(dg_overlay_host(s, frames.get(), W, H, n, items.data(), first.data()) == DG_OK);
    for (size_t i = 0; i < bytes; i++) CHECK(frames[i] == want[i]);
    if (check_plan(pics, W, H, n, items, first)) return 1;
    changed += bytes;
    return 0;
}

int main(int argc, char **argv) {
    CHECK(argc >= 4);
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    dg_scene *s = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[2], &s) == DG_OK);

    // ovl_div is `/` on its whole domain, and one past it on either side of the scale range
    for (uint32_t d = 1; d <= 16; d++) {
        const uint32_t m = dg::ovl_magic(d);
        for (uint32_t v = 0; v < (1u << 19) + 64u; v++) CHECK(dg::ovl_div(v, m) == v / d);
    }

    // the palette, from the WAD's directory (the last PLAYPAL)
    const uint8_t *palette = nullptr;
    {
        uint32_t nl, dir;
        std::memcpy(&nl, wad.data() + 4, 4); std::memcpy(&dir, wad.data() + 8, 4);
        for (uint32_t i = 0; i < nl; i++) {
            uint32_t off;
            std::memcpy(&off, wad.data() + dir + 16 * i, 4);
            if (std::strncmp((const char *)wad.data() + dir + 16 * i + 8, "PLAYPAL", 8) == 0) palette = wad.data() + off;
        }
    }
    CHECK(palette != nullptr);

    std::vector<Pic> pics;
    for (int a = 3; a < argc; a++) {
        Pic p{};
        p.handle = dg_scene_use_picture(s, argv[a]);
        CHECK(p.handle == a - 3 && dg_scene_use_picture(s, argv[a]) == p.handle);
        if (read_picture(s, palette, p)) return 1;
        pics.push_back(std::move(p));
    }
    CHECK(dg_scene_picture_count(s) == (int)pics.size());

    uint64_t bytes = 0;
    const int sizes[3][2] = {{5, 3}, {131, 67}, {1, 1}};
    for (const auto &wh : sizes) {
        const int W = wh[0], H = wh[1];
        for (size_t pi = 0; pi < pics.size(); pi++) {
            const Pic &p = pics[pi];
            for (const int sc : {1, 3, 16}) {
                const int pw = p.w * sc, ph = p.h * sc;
                // over every edge and corner, wholly inside (when it fits), wholly outside on each side, touching from outside
                const int xs[] = {-pw - 1, -pw, -pw + 1, -pw / 2, 0, (W - pw) / 2, W - pw / 2, W - 1, W, W + 1};
                const int ys[] = {-ph - 1, -ph, -ph + 1, -ph / 2, 0, (H - ph) / 2, H - ph / 2, H - 1, H, H + 1};
                std::vector<dg_screen_picture> items;
                std::vector<uint32_t> first{0};
                for (const int y : ys) {
                    for (const int x : xs) {
                        const uint16_t flags = (uint16_t)(rng() & 3u);
                        const int16_t light = (int16_t)(rng() % 256u);
                        items.push_back(dg_screen_picture{(int32_t)pi, x, y, (uint16_t)sc, (uint16_t)(sc == 3 ? 5 : sc), light, flags});
                        items.push_back(dg_screen_picture{(int32_t)((pi + 1) % pics.size()), x + 1, y - 1, 1, 2, 255, DG_PIC_OFFSETS});
                    }
                    first.push_back((uint32_t)items.size());
                    first.push_back((uint32_t)items.size());                   // a frame without items after every frame with some
                }
                if (run(s, pics, palette, W, H, (int)first.size() - 1, items, first, bytes)) return 1;
            }
        }
        // all of it in one frame: more items than a frame's bands are built from
        std::vector<dg_screen_picture> many;
        for (int i = 0; i < 100; i++)
            many.push_back(dg_screen_picture{(int32_t)(rng() % pics.size()), (int32_t)(rng() % (uint32_t)(W + 40)) - 20, (int32_t)(rng() % (uint32_t)(H + 40)) - 20,
                                             (uint16_t)(1 + rng() % 3), (uint16_t)(1 + rng() % 3), (int16_t)(rng() % 256u), (uint16_t)(rng() & 3u)});
        if (run(s, pics, palette, W, H, 1, many, {0, (uint32_t)many.size()}, bytes)) return 1;
    }

    // refusals leave the frame alone
    {
        std::unique_ptr<uint8_t[]> one(new uint8_t[3]);
        one[0] = 1; one[1] = 2; one[2] = 3;
        const uint32_t first[2] = {0, 1};
        dg_screen_picture bad{(int32_t)pics.size(), 0, 0, 1, 1, 255, 0};
        CHECK(dg_overlay_host(s, one.get(), 1, 1, 1, &bad, first) == DG_ERR_INVALID);
        bad = dg_screen_picture{0, 0, 0, 17, 1, 255, 0};
        CHECK(dg_overlay_host(s, one.get(), 1, 1, 1, &bad, first) == DG_ERR_INVALID);
        CHECK(one[0] == 1 && one[1] == 2 && one[2] == 3);
    }
    dg_scene_free(s);
    std::printf("overlay_host_main: ok (%llu frame bytes compared)\n", (unsigned long long)bytes);
    return 0;
}
