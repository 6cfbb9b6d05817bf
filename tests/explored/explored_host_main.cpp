// tests/explored/explored_host_main.cpp WAD PATH.f32 MAP — the host side of the explored-map frames as a stand-alone program, for a
// sanitizer build (tests/test_explored_host.py builds it with -fsanitize=address,undefined together with the library's host sources and
// runs it).  dg_seen_lines_host, dg_seen_accumulate_host and dg_explored_map_host through the C-ABI, with buffers of exactly the size the
// contract names, against the rules restated here as plain loops; and the structure the GPU draws from — build_explored_cover's cover and
// chains read through explored_pick — against dg_explored_map_host's literal draw loop, pixel for pixel.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/explored_cover.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("explored_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static uint32_t rng32() { return (rng() << 16) ^ rng(); }
static int popc(uint32_t v) { int n = 0; for (; v; v &= v - 1) n++; return n; }

static int check_seen(const dg_scene *s, int W, int H, int n, const std::vector<uint16_t> &id, const std::vector<uint8_t> &cls) {
    const dg::Scene &sc = *s->sc;
    const size_t words = (size_t)dg_seen_words(s), px = (size_t)W * (size_t)H;
    std::vector<uint32_t> seen((size_t)n * words, 0x5a5a5a5au);
    CHECK(dg_seen_lines_host(s, W, H, n, id.data(), cls.data(), seen.data()) == DG_OK);
    for (int f = 0; f < n; f++)
        for (size_t l = 0; l < words * 32; l++) {
            bool want = false;
            for (size_t p = 0; p < px && !want; p++) {
                const size_t q = (size_t)f * px + p;
                want = cls[q] == DG_LABEL_WALL && id[q] < sc.segs.size() && (size_t)sc.segs[id[q]].linedef == l;
            }
            CHECK((((seen[(size_t)f * words + (l >> 5)] >> (l & 31)) & 1u) != 0) == want);
        }
    return 0;
}

static int check_accumulate(int words, int n, int run_len, bool carry) {
    const int runs = n / run_len;
    const size_t Wd = (size_t)words;
    std::vector<uint32_t> seen((size_t)n * Wd), cin((size_t)runs * Wd), upto((size_t)n * Wd, 7u), total((size_t)n, 7u), fresh((size_t)n, 7u), cout((size_t)runs * Wd, 7u);
    for (uint32_t &v : seen) v = rng32() & rng32() & rng32();
    for (uint32_t &v : cin) v = rng32() & rng32();
    CHECK(dg_seen_accumulate_host(words, n, run_len, carry ? cin.data() : nullptr, seen.data(), upto.data(), total.data(), fresh.data(), cout.data()) == DG_OK);
    for (int f = 0; f < n; f++) {
        const int run = f / run_len;
        int t = 0, fr = 0;
        for (size_t w = 0; w < Wd; w++) {
            uint32_t acc = carry ? cin[(size_t)run * Wd + w] : 0u, prev = acc;
            for (int g = run * run_len; g <= f; g++) { prev = acc; acc |= seen[(size_t)g * Wd + w]; }
            CHECK(upto[(size_t)f * Wd + w] == acc);
            t += popc(acc); fr += popc(acc & ~prev);
            if (f == (run + 1) * run_len - 1) CHECK(cout[(size_t)run * Wd + w] == acc);
        }
        CHECK(total[(size_t)f] == (uint32_t)t && fresh[(size_t)f] == (uint32_t)fr);
    }
    // every output alone
    std::vector<uint32_t> one((size_t)n * Wd);
    CHECK(dg_seen_accumulate_host(words, n, run_len, carry ? cin.data() : nullptr, seen.data(), one.data(), nullptr, nullptr, nullptr) == DG_OK && one == upto);
    std::vector<uint32_t> cnt((size_t)n);
    CHECK(dg_seen_accumulate_host(words, n, run_len, carry ? cin.data() : nullptr, seen.data(), nullptr, cnt.data(), nullptr, nullptr) == DG_OK && cnt == total);
    CHECK(dg_seen_accumulate_host(words, n, run_len, carry ? cin.data() : nullptr, seen.data(), nullptr, nullptr, cnt.data(), nullptr) == DG_OK && cnt == fresh);
    std::vector<uint32_t> co((size_t)runs * Wd);
    CHECK(dg_seen_accumulate_host(words, n, run_len, carry ? cin.data() : nullptr, seen.data(), nullptr, nullptr, nullptr, co.data()) == DG_OK && co == cout);
    return 0;
}

static int check_frames(const dg_scene *s, int W, int H, const dg_view *view, uint64_t &pixels, uint64_t &chained) {
    const dg::Scene &sc = *s->sc;
    const size_t words = (size_t)dg_seen_words(s), px = (size_t)W * (size_t)H, L = sc.linedefs.size();
    dg::ExploredCover cv;
    std::string err;
    CHECK(dg::build_explored_cover(sc, W, H, cv, err) == DG_OK);
    CHECK(cv.cover.size() == px && !cv.chains.empty());
    for (size_t p = 0; p < px; p++) {                      // the structure: entries name drawn linedefs, a chain has >= 2 of them, the latest first
        const uint32_t c = cv.cover[p];
        if (c == 0) continue;
        const uint32_t *e = &c;
        uint32_t n = 1;
        if (c & dg::EXPLORED_CHAIN) {
            const size_t at = c & ~dg::EXPLORED_CHAIN;
            CHECK(at < cv.chains.size());
            n = cv.chains[at];
            CHECK(n >= 2 && at + n < cv.chains.size());
            e = &cv.chains[at + 1];
            chained++;
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t line = (e[i] & dg::EXPLORED_LINE) - 1u;
            CHECK(line < L && !(sc.linedefs[line].flags & 128));
            CHECK(((e[i] & dg::EXPLORED_YELLOW) != 0) == ((sc.linedefs[line].flags & 4) != 0));
            if (i) CHECK(line < (e[i - 1] & dg::EXPLORED_LINE) - 1u);
        }
    }
    std::vector<uint8_t> frame(3 * px);
    for (int m = 0; m < 7; m++) {
        std::vector<uint32_t> mask(words);
        for (size_t w = 0; w < words; w++) mask[w] = m == 0 ? 0xffffffffu : m == 1 ? 0u : m == 2 ? 0x55555555u : m == 3 ? 0xaaaaaaaau : m == 4 ? rng32() : m == 5 ? rng32() & rng32() : rng32() | rng32();
        if (L % 32) mask[words - 1] &= (1u << (L % 32)) - 1u;
        CHECK(dg_explored_map_host(s, W, H, nullptr, mask.data(), frame.data()) == DG_OK);
        for (size_t p = 0; p < px; p++) {
            const uint32_t rgb = dg::explored_pick(cv.cover[p], cv.chains.data(), mask.data());
            CHECK(frame[3 * p] == (uint8_t)rgb && frame[3 * p + 1] == (uint8_t)(rgb >> 8) && frame[3 * p + 2] == (uint8_t)(rgb >> 16));
            pixels++;
        }
        if (m == 0 && view) {                              // all ones + arrow == dg_map_lines drawn in order
            const int n = dg_map_lines(s, W, H, view, nullptr, 0);
            CHECK(n >= 3);
            std::vector<dg_map_line> lines((size_t)n);
            CHECK(dg_map_lines(s, W, H, view, lines.data(), n) == n);
            std::vector<uint8_t> want(3 * px, 0), got(3 * px);
            for (const dg_map_line &l : lines) {
                const dg::MapSeg sg = dg::map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
                for (int32_t i = 0; i < sg.count; i++) {
                    int32_t x, y;
                    dg::map_seg_point(sg, (int64_t)sg.first + i, x, y);
                    CHECK(x >= 0 && x < W && y >= 0 && y < H);
                    uint8_t *o = &want[3 * ((size_t)y * (size_t)W + (size_t)x)];
                    o[0] = (uint8_t)l.rgb; o[1] = (uint8_t)(l.rgb >> 8); o[2] = (uint8_t)(l.rgb >> 16);
                }
            }
            CHECK(dg_explored_map_host(s, W, H, view, mask.data(), got.data()) == DG_OK && got == want);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::printf("usage: explored_host_main WAD PATH.f32 MAP\n"); return 2; }
    std::ifstream wf(argv[1], std::ios::binary), pf(argv[2], std::ios::binary);
    std::vector<char> wad((std::istreambuf_iterator<char>(wf)), std::istreambuf_iterator<char>()), pb((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
    CHECK(!wad.empty() && pb.size() >= 1000 * 8 * sizeof(float));
    const float *path = reinterpret_cast<const float *>(pb.data());
    dg_scene *s = nullptr;
    CHECK(dg_scene_load_wad(reinterpret_cast<const uint8_t *>(wad.data()), wad.size(), argv[3], &s) == DG_OK);
    const dg::Scene &sc = *s->sc;
    const int words = dg_seen_words(s);
    CHECK(words == (int)((sc.linedefs.size() + 31) / 32) && words >= 1);
    auto view_of = [&](int i) {
        const float *r = path + 8 * i;
        return dg_view{r[0], r[1], r[2], r[7], r[3], r[4], r[5], r[6], 0.0f, 1};
    };
    // seen rows: label planes of path views, then synthetic planes
    const int idx[] = {0, 297, 623};
    for (auto &sz : {std::pair<int, int>{131, 67}, {44, 41}}) {
        const int W = sz.first, H = sz.second;
        const size_t px = (size_t)W * (size_t)H;
        std::vector<uint16_t> id(3 * px);
        std::vector<uint8_t> cls(3 * px);
        for (int k = 0; k < 3; k++) {
            const dg_view v = view_of(idx[k]);
            dg_frame_lists fl;
            const uint32_t *owners = nullptr;
            CHECK(dg_build_lists_owners(s, W, H, &v, &fl, &owners) == DG_OK);
            CHECK(dg_label_lists_host(s, W, H, &fl, &owners, 1, id.data() + (size_t)k * px, cls.data() + (size_t)k * px, nullptr) == DG_OK);
        }
        if (check_seen(s, W, H, 3, id, cls)) return 1;
        const uint32_t S = (uint32_t)sc.segs.size();
        for (size_t p = 0; p < 3 * px; p++) {
            const uint32_t r = rng();
            cls[p] = (uint8_t)(r % 5u);
            id[p] = (uint16_t)(r % 7u == 0 ? S + (r >> 3) % 3u : (r >> 3) % 64u == 0 ? 65535u : (r >> 3) % S);
        }
        id[0] = 31; cls[0] = DG_LABEL_WALL; id[1] = 32; cls[1] = DG_LABEL_WALL; id[2] = (uint16_t)(S - 1); cls[2] = DG_LABEL_WALL;
        if (check_seen(s, W, H, 3, id, cls)) return 1;
    }
    // accumulation
    for (int w : {1, 17})
        for (int n : {1, 12})
            for (int run_len : {1, 4, 12})
                if (n % run_len == 0)
                    for (bool carry : {false, true})
                        if (check_accumulate(w, n, run_len, carry)) return 1;
    // frames: the cover and explored_pick against the literal rule
    uint64_t pixels = 0, chained = 0;
    const dg_view v = view_of(500);
    for (auto &sz : {std::pair<int, int>{64, 40}, {44, 41}, {131, 67}, {320, 200}})
        if (check_frames(s, sz.first, sz.second, &v, pixels, chained)) return 1;
    CHECK(chained > 0);
    // the error returns: nothing is read or written (every buffer below is one element)
    uint16_t i1 = 0; uint8_t c1 = 0, px1[3] = {9, 9, 9}; uint32_t r1 = 77;
    std::vector<uint32_t> row((size_t)words, 0xffffffffu);
    CHECK(dg_seen_words(nullptr) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(nullptr, 1, 1, 1, &i1, &c1, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 0, 1, 1, &i1, &c1, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 1, 16385, 1, &i1, &c1, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 1, 1, -1, &i1, &c1, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 1, 1, 1, nullptr, &c1, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 1, 1, 1, &i1, nullptr, row.data()) == DG_ERR_INVALID);
    CHECK(dg_seen_lines_host(s, 1, 1, 1, &i1, &c1, nullptr) == DG_ERR_INVALID);
    CHECK(row[0] == 0xffffffffu);
    CHECK(dg_seen_lines_host(s, 1, 1, 0, &i1, &c1, row.data()) == DG_OK && row[0] == 0xffffffffu);
    CHECK(dg_seen_accumulate_host(0, 1, 1, nullptr, &r1, &r1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_seen_accumulate_host(1, -1, 1, nullptr, &r1, &r1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_seen_accumulate_host(1, 1, 0, nullptr, &r1, &r1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_seen_accumulate_host(1, 3, 2, nullptr, &r1, &r1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_seen_accumulate_host(1, 1, 1, nullptr, nullptr, &r1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(r1 == 77);
    CHECK(dg_seen_accumulate_host(1, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DG_OK);
    CHECK(dg_seen_accumulate_host(1, 1, 1, nullptr, &r1, nullptr, nullptr, nullptr, nullptr) == DG_OK);
    CHECK(dg_explored_map_host(nullptr, 40, 40, nullptr, row.data(), px1) == DG_ERR_INVALID);
    CHECK(dg_explored_map_host(s, 40, 40, nullptr, nullptr, px1) == DG_ERR_INVALID);
    CHECK(dg_explored_map_host(s, 40, 40, nullptr, row.data(), nullptr) == DG_ERR_INVALID);
    CHECK(dg_explored_map_host(s, 39, 40, nullptr, row.data(), px1) == DG_ERR_INVALID);
    const dg_view far{1e12f, 0.0f, 0.0f, 0.0f, 0, 0, 0, 0, 0.0f, 0};
    CHECK(dg_explored_map_host(s, 64, 64, &far, row.data(), px1) == DG_ERR_INVALID);       // (not at 40 x 40: every point lands on the border there)
    CHECK(px1[0] == 9 && px1[1] == 9 && px1[2] == 9);
    dg_scene_free(s);
    std::printf("explored_host_main: ok (%llu pixels picked, %llu of them through a chain)\n", (unsigned long long)pixels, (unsigned long long)chained);
    return 0;
}
