// tests/labels/label_host_main.cpp — the host side of the object-label frame as a stand-alone program, for a sanitizer build
// (tests/test_labels_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
//   usage: label_host_main <wad file> <camera path .f32> <map name>
// Through the C-ABI alone: dg_build_lists_owners for path frames at several sizes, dg_label_lists_host on their lists and on lists with
// hand-given owners, every refused tag.  It checks what it gets: planes and boxes must agree with each other, a refused call writes nothing.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/doomgpu.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("label_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

// Planes against boxes: every class-2 pixel lies inside its object's box and the counts add up; ids are 0 outside classes 1 and 2.
static int consistent(int W, int H, int n_mobjs, const std::vector<uint16_t> &id, const std::vector<uint8_t> &cls, const std::vector<dg_label_box> &boxes) {
    std::vector<uint32_t> count((size_t)n_mobjs, 0u);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * (size_t)W + (size_t)x;
            CHECK(cls[i] <= DG_LABEL_SKY);
            if (cls[i] != DG_LABEL_WALL && cls[i] != DG_LABEL_MOBJ) CHECK(id[i] == 0);
            if (cls[i] != DG_LABEL_MOBJ) continue;
            CHECK(id[i] < n_mobjs);
            const dg_label_box &b = boxes[id[i]];
            CHECK(x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1);
            count[id[i]]++;
        }
    for (int m = 0; m < n_mobjs; m++) {
        CHECK(boxes[(size_t)m].pixels == count[(size_t)m]);
        if (!count[(size_t)m]) CHECK(boxes[(size_t)m].x0 == -1 && boxes[(size_t)m].y0 == -1 && boxes[(size_t)m].x1 == -1 && boxes[(size_t)m].y1 == -1);
    }
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
    CHECK(n_mobjs > 0);
    const int sizes[][2] = {{160, 100}, {131, 67}, {5, 9}, {64, 200}};
    uint64_t mobj_pixels = 0, frames = 0;
    for (auto &s : sizes) {
        const int W = s[0], H = s[1];
        const size_t px = (size_t)W * (size_t)H;
        std::vector<uint16_t> id(2 * px);
        std::vector<uint8_t> cls(2 * px);
        std::vector<dg_label_box> boxes(2 * (size_t)n_mobjs);
        for (int i = 0; i < 1000; i += 111) {
            const float *r = &path[(size_t)i * 8];
            const dg_view v{r[0], r[1], r[2], r[7], r[3], r[4], r[5], r[6], 0.0f, 1};
            dg_frame_lists fl;
            const uint32_t *owners = nullptr;
            CHECK(dg_build_lists_owners(sc, W, H, &v, &fl, &owners) == DG_OK);
            CHECK(fl.n_renders == 0 || owners != nullptr);
            // the frame twice in one call: as built, and with hand-given owners (every record the last map object's)
            std::vector<uint32_t> hand(fl.n_renders, ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)(n_mobjs - 1));
            const dg_frame_lists two[2] = {fl, fl};
            const uint32_t *const own2[2] = {owners, hand.data()};
            std::vector<uint32_t> keep(owners, owners + fl.n_renders);          // (the arena may move: the call below bins, it does not build)
            CHECK(dg_label_lists_host(sc, W, H, two, own2, 2, id.data(), cls.data(), boxes.data()) == DG_OK);
            for (int k = 0; k < 2; k++) {
                const std::vector<uint16_t> i1(id.begin() + (ptrdiff_t)(k * px), id.begin() + (ptrdiff_t)((k + 1) * px));
                const std::vector<uint8_t> c1(cls.begin() + (ptrdiff_t)(k * px), cls.begin() + (ptrdiff_t)((k + 1) * px));
                const std::vector<dg_label_box> b1(boxes.begin() + (ptrdiff_t)k * n_mobjs, boxes.begin() + (ptrdiff_t)(k + 1) * n_mobjs);
                if (consistent(W, H, n_mobjs, i1, c1, b1)) return 1;
                for (const dg_label_box &b : b1) mobj_pixels += b.pixels;
            }
            for (size_t p = 0; p < px; p++)                                       // hand-given owners change ids and classes 1 <-> 2, nothing else
                CHECK((cls[p] == DG_LABEL_WALL || cls[p] == DG_LABEL_MOBJ) == (cls[px + p] == DG_LABEL_MOBJ) && (cls[px + p] != DG_LABEL_MOBJ || id[px + p] == n_mobjs - 1));
            // refused tags: nothing is written
            if (fl.n_renders) {
                const uint32_t bad_tags[] = {0u, 3u << 16, ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)n_mobjs, ((uint32_t)DG_LABEL_WALL << 16) | 0xffffu, 0xffffffffu};
                for (uint32_t t : bad_tags) {
                    std::vector<uint32_t> bad(keep);
                    bad.back() = t;
                    const uint32_t *const ob[2] = {keep.data(), bad.data()};
                    std::vector<uint8_t> c2(2 * px, 77);
                    CHECK(dg_label_lists_host(sc, W, H, two, ob, 2, nullptr, c2.data(), nullptr) == DG_ERR_INVALID);
                    for (uint8_t c : c2) CHECK(c == 77);
                }
                const uint32_t *const on[2] = {keep.data(), nullptr};
                CHECK(dg_label_lists_host(sc, W, H, two, on, 2, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
            }
            CHECK(dg_label_lists_host(sc, W, H, two, own2, 2, nullptr, nullptr, nullptr) == DG_OK);
            frames++;
        }
    }
    CHECK(mobj_pixels > 0);
    dg_scene_free(sc);
    std::printf("label_host_main: ok (%llu frames, %llu map-object pixels)\n", (unsigned long long)frames, (unsigned long long)mobj_pixels);
    return 0;
}
