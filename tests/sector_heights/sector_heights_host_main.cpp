// tests/sector_heights/sector_heights_host_main.cpp — the per-view sector heights' host side as a stand-alone program, for a sanitizer
// build (tests/test_sector_heights_host.py builds it with -fsanitize=address,undefined together with the library's host sources and
// runs it).
//   usage: sector_heights_host_main <wad file> <camera path .f32> <map name>
// resolve_view_sectors over duplicate, out-of-range and out-of-int16 entries; view_rows_core.h's fill and scatter bodies lane after
// lane, as the two kernels index them (256-lane groups, the last one partial), over batches and entry counts at the kernels'
// boundaries, every row compared with the entries applied in order; then the host walker with entries through the C-ABI.  It checks
// what it gets.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/frontend.hpp"
#include "../../doom-rust-renderer_amd/csrc/slab_layout.h"
#include "../../doom-rust-renderer_amd/csrc/view_rows_core.h"

using namespace dg;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("sector_heights_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rnd(uint32_t &s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
static int32_t height(uint32_t &s) {
    const uint32_t k = rnd(s) % 16;
    return k == 0 ? -32768 : k == 1 ? 32767 : (int32_t)(rnd(s) % 1201) - 600;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), {});
    std::ifstream pf(argv[2], std::ios::binary);
    std::vector<float> path(8000);
    pf.read((char *)path.data(), 32000);
    dg_scene *h = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[3], &h) == DG_OK);
    const Scene &sc = *h->sc;
    const uint32_t n_sectors = (uint32_t)sc.sectors.size();
    CHECK(n_sectors > 0 && sc.fs_heights.size() == n_sectors);
    {
        std::vector<int16_t> fl(n_sectors), ce(n_sectors);
        CHECK(dg_scene_sector_heights(h, fl.data(), ce.data(), (int)n_sectors) == DG_OK);
        for (uint32_t s = 0; s < n_sectors; s++) CHECK(fl[s] == sc.sectors[s].floor_h && ce[s] == sc.sectors[s].ceil_h && sc.fs_heights[s].floor_h == fl[s] && sc.fs_heights[s].ceil_h == ce[s]);
        CHECK(dg_scene_sector_heights(h, fl.data(), ce.data(), (int)n_sectors + 1) == DG_ERR_INVALID);
    }

    // resolve_view_sectors: the later of two wins, bad entries are reported and left out, the index row is handed back clean
    LatestHeights latest;
    std::vector<int32_t> &height_of = latest.of;
    std::vector<dg_sector_heights> &stand = latest.out;
    {
        const dg_sector_heights in[] = {{3, 500, -300}, {0, 1, 2}, {3, 8, 8}, {(int32_t)n_sectors, 0, 0}, {-1, 0, 0}, {1, 32768, 0}, {1, 0, -32769}, {2, -32768, 32767}};
        const dg_view_sectors vs{in, 8};
        CHECK(resolve_view_sectors(sc, vs, latest) == 3u);
        CHECK(stand.size() == 3 && stand[0].sector == 3 && stand[0].floor_height == 8 && stand[0].ceiling_height == 8 && stand[1].sector == 0 && stand[2].sector == 2);
        CHECK(height_of[3] == 0 && height_of[0] == 1 && height_of[2] == 2 && height_of[1] == -1);
        latest.release();
        for (int32_t v : height_of) CHECK(v == -1);
        const dg_view_sectors none{nullptr, 0};
        CHECK(resolve_view_sectors(sc, none, latest) == 0u && stand.empty());
    }

    // LatestPerIndex, what the three resolve_view_* de-duplicate with: a repeated index keeps the place of its first entry and the
    // value of its last, release() hands the index row back all -1 and leaves out alone, begin() with another item count re-sizes
    {
        struct Item { int32_t index; int value; };
        LatestPerIndex<Item, &Item::index> l;
        l.begin(5);
        CHECK(l.of.size() == 5 && l.out.empty());
        for (int32_t v : l.of) CHECK(v == -1);
        for (const Item &it : {Item{4, 40}, Item{1, 10}, Item{4, 41}, Item{0, 7}, Item{1, 11}, Item{4, 42}}) l.put(it);
        CHECK(l.out.size() == 3 && l.out[0].index == 4 && l.out[0].value == 42 && l.out[1].index == 1 && l.out[1].value == 11 && l.out[2].index == 0 && l.out[2].value == 7);
        CHECK(l.of[4] == 0 && l.of[1] == 1 && l.of[0] == 2 && l.of[2] == -1 && l.of[3] == -1);
        l.release();
        for (int32_t v : l.of) CHECK(v == -1);
        CHECK(l.of.size() == 5 && l.out.size() == 3 && l.out[0].value == 42);
        l.release();                                                    // (a second one changes nothing)
        for (int32_t v : l.of) CHECK(v == -1);
        l.begin(5);
        CHECK(l.out.empty() && l.of.size() == 5);
        l.put(Item{4, 1});
        CHECK(l.of[4] == 0 && l.out.size() == 1);                       // (the first place again, not the earlier view's)
        l.release();
        l.begin(9);
        CHECK(l.of.size() == 9 && l.out.empty());
        for (int32_t v : l.of) CHECK(v == -1);
        l.put(Item{8, 80}); l.put(Item{8, 81}); l.put(Item{0, 1});
        CHECK(l.of[8] == 0 && l.of[0] == 1 && l.out.size() == 2 && l.out[0].value == 81);
        l.release();
        for (int32_t v : l.of) CHECK(v == -1);
        l.begin(2);
        CHECK(l.of.size() == 2 && l.out.empty());
        for (int32_t v : l.of) CHECK(v == -1);
        l.begin(0);
        CHECK(l.of.empty() && l.out.empty());
    }

    // the row bodies at the kernels' boundary counts
    uint32_t seed = 88172645u;
    uint64_t cells_checked = 0;
    for (uint32_t n_frames : {1u, 3u, 64u, 65u}) {
        const SectorRowLayout L = sector_row_layout(n_frames, n_sectors);
        const uint32_t total = n_frames * n_sectors;
        CHECK(L.cells == total && L.rows == (size_t)total * 4 && L.entries == (size_t)total * 12);
        for (uint32_t want_entries : {0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, total}) {
            const uint32_t n_entries = want_entries < total ? want_entries : total;
            // the caller's entries per frame (with a losing earlier entry for every fifth), resolved into the staging as build_batch_fs does
            std::vector<std::vector<dg_sector_heights>> given(n_frames);
            std::vector<uint8_t> used(total, 0);
            for (uint32_t e = 0; e < n_entries; e++) {
                uint32_t cell = n_entries == total ? e : rnd(seed) % total;
                while (used[cell]) cell = (cell + 1) % total;
                used[cell] = 1;
                const int32_t s = (int32_t)(cell % n_sectors);
                if (e % 5 == 0) given[cell / n_sectors].push_back(dg_sector_heights{s, 12345, -12345});
                given[cell / n_sectors].push_back(dg_sector_heights{s, height(seed), height(seed)});
            }
            std::vector<SectorEntry> staged(L.cells);
            std::vector<FsHeights> want(total);
            uint32_t n_staged = 0;
            for (uint32_t fr = 0; fr < n_frames; fr++) {
                for (uint32_t s = 0; s < n_sectors; s++) want[fr * n_sectors + s] = sc.fs_heights[s];
                for (const dg_sector_heights &g : given[fr]) want[fr * n_sectors + (uint32_t)g.sector] = FsHeights{(int16_t)g.floor_height, (int16_t)g.ceiling_height};
                const dg_view_sectors vs{given[fr].data(), (uint32_t)given[fr].size()};
                CHECK(resolve_view_sectors(sc, vs, latest) == 0u);
                for (const dg_sector_heights &g : stand) { CHECK(n_staged < L.cells); staged[n_staged++] = SectorEntry{(int32_t)fr, g.sector, (int16_t)g.floor_height, (int16_t)g.ceiling_height}; }
                latest.release();
            }
            CHECK(n_staged == n_entries);
            std::vector<FsHeights> rows(total, FsHeights{-1, -1});
            const SectorRowParams P{sc.fs_heights.data(), staged.data(), rows.data(), n_sectors, n_frames, n_staged};
            for (uint32_t b = 0; b < (total + 255u) / 256u; b++)
                for (uint32_t t = 0; t < 256; t++)
                    if (b * 256u + t < P.n_frames * P.n_items) view_row_fill(P, b * 256u + t);
            for (uint32_t b = 0; b < (n_staged + 255u) / 256u; b++)
                for (uint32_t t = 0; t < 256; t++)
                    if (b * 256u + t < P.n_entries) view_row_scatter(P, b * 256u + t);
            CHECK(std::memcmp(rows.data(), want.data(), (size_t)total * sizeof(FsHeights)) == 0);
            cells_checked += total;
        }
    }
    {   // an entry outside the batch is left alone (the host has checked both; the body checks again)
        std::vector<FsHeights> rows(2 * n_sectors, FsHeights{7, 7});
        const SectorEntry bad[] = {{2, 0, 1, 1}, {-1, 0, 1, 1}, {0, (int32_t)n_sectors, 1, 1}, {0, -1, 1, 1}, {1, (int32_t)n_sectors - 1, 5, 6}};
        const SectorRowParams P{sc.fs_heights.data(), bad, rows.data(), n_sectors, 2, 5};
        for (uint32_t e = 0; e < 5; e++) view_row_scatter(P, e);
        for (uint32_t i = 0; i + 1 < 2 * n_sectors; i++) CHECK(rows[i].floor_h == 7 && rows[i].ceil_h == 7);
        CHECK(rows[2 * n_sectors - 1].floor_h == 5 && rows[2 * n_sectors - 1].ceil_h == 6);
    }

    // the host walker with entries, through the C-ABI
    uint64_t renders = 0, changed = 0;
    for (int fr : {40, 323, 640, 817}) {
        dg_view v{};
        const float *r = path.data() + 8 * fr;
        v.x = r[0]; v.y = r[1]; v.angle = r[2]; v.floor_height = r[7];
        dg_frame_lists plain{}, fl{};
        CHECK(dg_build_lists(h, 160, 100, &v, &plain) == DG_OK);
        const uint32_t n_plain = plain.n_renders, n_plain_planes = plain.n_visplanes;
        std::vector<dg_sector_heights> all;
        for (uint32_t s = 0; s < n_sectors; s++) all.push_back(dg_sector_heights{(int32_t)s, height(seed), height(seed)});
        const dg_view_sectors vs{all.data(), (uint32_t)all.size()};
        const uint32_t *owners = nullptr;
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, &vs, &fl, &owners) == DG_OK);
        renders += fl.n_renders;
        changed += fl.n_renders != n_plain || fl.n_visplanes != n_plain_planes;
        const dg_view_sectors none{nullptr, 0};
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, &none, &fl, nullptr) == DG_OK && fl.n_renders == n_plain && fl.n_visplanes == n_plain_planes);
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, nullptr, &fl, nullptr) == DG_OK && fl.n_renders == n_plain);
        const dg_sector_heights wild{(int32_t)n_sectors, 0, 0}, tall{0, 40000, 0};
        const dg_view_sectors w{&wild, 1}, t{&tall, 1}, null_arr{nullptr, 2};
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, &w, &fl, nullptr) == DG_ERR_INVALID);
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, &t, &fl, nullptr) == DG_ERR_INVALID);
        CHECK(dg_build_lists_sectors(h, 160, 100, &v, nullptr, &null_arr, &fl, nullptr) == DG_ERR_INVALID);
    }
    CHECK(renders > 0 && changed > 0 && cells_checked > 0);
    dg_scene_free(h);
    std::printf("sector_heights_host_main: ok (%llu cells, %llu renders)\n", (unsigned long long)cells_checked, (unsigned long long)renders);
    return 0;
}
