// tests/surfaces/surfaces_host_main.cpp — the per-view surfaces' host side as a stand-alone program, for a sanitizer build
// (tests/test_surfaces_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
//   usage: surfaces_host_main <wad file> <camera path .f32> <map name>
// resolve_view_surfaces over duplicate and invalid entries; view_rows_core.h's fill and scatter bodies lane after lane, as the two
// kernels index them (256-lane groups, the last one partial), over batches and entry counts at the kernels' boundaries; fs_side_find
// over 0, 1, 2 and 257 entries with hits at both ends and misses below, between and above; the side table laid out as build_batch_fs
// stages it; then the host walker with entries through the C-ABI.  It checks what it gets.
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
        if (!(cond)) { std::printf("surfaces_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rnd(uint32_t &s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), {});
    std::ifstream pf(argv[2], std::ios::binary);
    std::vector<float> path(8000);
    pf.read((char *)path.data(), 32000);
    dg_scene *h = nullptr;
    CHECK(dg_scene_load_wad(wad.data(), wad.size(), argv[3], &h) == DG_OK);
    const int t_brick = dg_scene_use_texture(h, "BRICK1"), t_grate = dg_scene_use_texture(h, "GRATE1"), t_wide = dg_scene_use_texture(h, "wide2");
    const int f_floor = dg_scene_use_flat(h, "FLOOR0"), f_sky = dg_scene_use_flat(h, "F_SKY1"), f_nuk = dg_scene_use_flat(h, "NUKAGE2");
    CHECK(t_brick >= 0 && t_grate >= 0 && t_wide >= 0 && f_floor >= 0 && f_sky >= 0 && f_nuk >= 0);
    CHECK(dg_scene_use_texture(h, "-") == DG_TEX_NONE && dg_scene_use_texture(h, "NOSUCHTX") == DG_ERR_WAD && dg_scene_use_flat(h, "NOSUCHFL") == DG_ERR_WAD);
    CHECK((f_sky & FS_FLAT_SKY) && !(f_floor & FS_FLAT_SKY) && (f_nuk & FS_FLAT_ANIM) && f_nuk == dg_scene_use_flat(h, "NUKAGE1"));
    const Scene &sc = *h->sc;
    const uint32_t n_sectors = (uint32_t)sc.sectors.size(), n_sides = (uint32_t)sc.sidedefs.size();
    CHECK(n_sectors > 0 && n_sides > 2 && sc.fs_flats.size() == n_sectors && sc.fs_seg_side.size() == sc.segs.size() && (int)n_sides == dg_scene_sidedef_count(h));
    {
        std::vector<dg_side_surface> sd(n_sides);
        std::vector<dg_sector_flats> fl(n_sectors);
        CHECK(dg_scene_sidedef_surfaces(h, sd.data(), (int)n_sides) == DG_OK && dg_scene_sector_flats(h, fl.data(), (int)n_sectors) == DG_OK);
        for (uint32_t i = 0; i < n_sides; i++) CHECK(sd[i].sidedef == (int32_t)i && sd[i].tex_mid == sc.sidedefs[i].middle && sd[i].x_offset == (int32_t)sc.sidedefs[i].xoff);
        for (uint32_t s = 0; s < n_sectors; s++) CHECK(fl[s].sector == (int32_t)s && sc.is_flat_handle(fl[s].floor_flat) && sc.is_flat_handle(fl[s].ceil_flat));
        CHECK(dg_scene_sidedef_surfaces(h, sd.data(), (int)n_sides + 1) == DG_ERR_INVALID && dg_scene_sector_flats(h, fl.data(), (int)n_sectors - 1) == DG_ERR_INVALID);
        for (size_t i = 0; i < sc.segs.size(); i++) CHECK(sc.fs_seg_side[i] >= -1 && sc.fs_seg_side[i] < (int32_t)n_sides && (sc.fs_seg_side[i] < 0) == (sc.fs_segs[i].front_sector < 0));
    }

    // resolve_view_surfaces: the later of two wins, bad entries are reported and left out, the output is sorted, the scratch handed back clean
    LatestSides latest_sides;
    LatestFlats latest_flats;
    std::vector<int32_t> &side_of = latest_sides.of, &flat_of = latest_flats.of;
    std::vector<FsSideEntry> &sides = latest_sides.out;
    std::vector<FlatEntry> &flats = latest_flats.out;
    {
        const dg_side_surface in[] = {{5, t_wide, t_wide, t_wide, 99, -99}, {2, t_brick, -1, t_grate, 1, 2}, {5, t_brick, t_brick, -1, -32768, 32767}, {(int32_t)n_sides, -1, -1, -1, 0, 0},
                                      {-1, -1, -1, -1, 0, 0}, {1, -2, -1, -1, 0, 0}, {1, -1, 1 << 24, -1, 0, 0}, {1, -1, -1, -1, 32768, 0}, {1, -1, -1, -1, 0, -32769}, {0, -1, -1, -1, 0, 0}};
        const dg_sector_flats fin[] = {{3, f_sky, f_sky}, {0, f_floor, f_nuk}, {3, f_nuk, f_floor}, {(int32_t)n_sectors, f_floor, f_floor}, {-1, f_floor, f_floor}, {1, -1, f_floor},
                                       {1, f_floor, FS_FLAT_MISSING}, {1, f_floor | FS_FLAT_SKY, f_floor}, {1, FS_FLAT_ANIM | 100000, f_floor}};
        const dg_view_surfaces vs{in, 10, fin, 9};
        CHECK(resolve_view_surfaces(sc, nullptr, vs, 7, latest_sides, latest_flats) == (1u | 2u | 4u | 8u | 16u));
        CHECK(sides.size() == 3 && sides[0].sidedef == 0 && sides[1].sidedef == 2 && sides[2].sidedef == 5 && sides[2].tex_mid == t_brick && sides[2].tex_up == -1 &&
              sides[2].x_offset == -32768 && sides[2].y_offset == 32767 && sides[1].anim_mid == -1);
        CHECK(flats.size() == 2 && flats[0].sector == 0 && flats[1].sector == 3 && flats[1].flats.floor == f_nuk && flats[1].flats.ceil == f_floor && flats[0].frame == 7);
        for (int32_t v : side_of) CHECK(v == -1);
        for (int32_t v : flat_of) CHECK(v == -1);
        const dg_view_surfaces none{nullptr, 0, nullptr, 0}, null_sides{nullptr, 2, nullptr, 0}, null_flats{nullptr, 0, nullptr, 1};
        CHECK(resolve_view_surfaces(sc, nullptr, none, 0, latest_sides, latest_flats) == 0u && sides.empty() && flats.empty());
        CHECK(resolve_view_surfaces(sc, nullptr, null_sides, 0, latest_sides, latest_flats) == 32u && resolve_view_surfaces(sc, nullptr, null_flats, 0, latest_sides, latest_flats) == 32u);
    }

    // the search: 0, 1, 2 and 257 entries; hits at both ends, misses below, between and above
    {
        for (uint32_t n : {0u, 1u, 2u, 257u}) {
            std::vector<FsSideEntry> e(n);
            for (uint32_t i = 0; i < n; i++) { e[i] = FsSideEntry{}; e[i].sidedef = 10 + 3 * (int32_t)i; }
            CHECK(fs_side_find(e.data(), n, 9) == -1 && fs_side_find(e.data(), n, -5) == -1 && fs_side_find(e.data(), n, 10 + 3 * (int32_t)n) == -1 && fs_side_find(e.data(), n, 1 << 30) == -1);
            for (uint32_t i = 0; i < n; i++) {
                CHECK(fs_side_find(e.data(), n, e[i].sidedef) == (int32_t)i);
                CHECK(fs_side_find(e.data(), n, e[i].sidedef + 1) == -1 && fs_side_find(e.data(), n, e[i].sidedef - 1) == -1);
            }
        }
    }

    uint32_t seed = 88172645u;
    // the side table as build_batch_fs stages it — first[frame], then the frames' sorted spans one after the other — searched as the
    // kernels' policy searches it (fs_surf_kernels.hip fs_surf_policy): frames without entries between frames that have them, every
    // seg of every frame asked
    uint64_t segs_asked = 0, segs_hit = 0;
    {
        const uint32_t counts[] = {0, 3, 0, 64, 1, 0, 2};
        const uint32_t n_frames = 7;
        const SurfaceLayout L = surface_layout(n_frames, n_sectors);
        std::vector<uint8_t> table(L.table);
        uint32_t *const first = reinterpret_cast<uint32_t *>(table.data());
        FsSideEntry *const se = reinterpret_cast<FsSideEntry *>(table.data() + L.first_bytes);
        std::vector<std::vector<dg_side_surface>> given(n_frames);
        uint32_t staged = 0;
        for (uint32_t fr = 0; fr < n_frames; fr++) {
            for (uint32_t k = 0; k < counts[fr]; k++) {
                const int32_t sd = k == 0 ? 0 : k == 1 ? (int32_t)n_sides - 1 : (int32_t)(rnd(seed) % n_sides);   // (both ends of the index range, then anywhere; a repeat loses to the later)
                given[fr].push_back(dg_side_surface{sd, t_wide, t_brick, t_grate, (int32_t)(fr * 100 + k), -(int32_t)k});
            }
            const dg_view_surfaces vs{given[fr].data(), (uint32_t)given[fr].size(), nullptr, 0};
            CHECK(resolve_view_surfaces(sc, nullptr, vs, (int32_t)fr, latest_sides, latest_flats) == 0u);
            CHECK(staged + sides.size() <= L.side_cap);
            first[fr] = staged;
            for (const FsSideEntry &e : sides) se[staged++] = e;
        }
        first[n_frames] = staged;
        for (uint32_t fr = 0; fr < n_frames; fr++) {
            CHECK(first[fr] <= first[fr + 1] && first[fr + 1] - first[fr] <= counts[fr]);
            for (uint32_t k = first[fr]; k + 1 < first[fr + 1]; k++) CHECK(se[k].sidedef < se[k + 1].sidedef);
            const FsViewSurfaces sf{sc.fs_flats.data(), se + first[fr], first[fr + 1] - first[fr], sc.fs_seg_side.data()};
            for (uint32_t si = 0; si < sc.fs_segs.size(); si++) {
                const FsSeg &sg = sc.fs_segs[si];
                const FsSeg got = sf.seg(FsNoFx(), sg, si, 0.0f);
                const dg_side_surface *want = nullptr;                              // the later of the frame's entries for this seg's sidedef
                for (const dg_side_surface &g : given[fr])
                    if (g.sidedef == sc.fs_seg_side[si]) want = &g;
                segs_asked++;
                if (want) {
                    segs_hit++;
                    CHECK(got.tex_mid == t_wide && got.tex_low == t_brick && got.tex_up == t_grate && got.sd_xoff == (float)want->x_offset && got.sd_yoff == (float)want->y_offset);
                    CHECK(got.v1x == sg.v1x && got.front_sector == sg.front_sector && got.seg_offset == sg.seg_offset && got.ld_flags == sg.ld_flags);
                } else {
                    CHECK(std::memcmp(&got, &sg, sizeof sg) == 0);
                }
            }
        }
        CHECK(segs_hit > 0 && segs_hit < segs_asked);
    }

    // the row bodies at the kernels' boundary counts
    uint64_t cells_checked = 0;
    const int32_t handles[] = {f_floor, f_sky, f_nuk};
    for (uint32_t n_frames : {1u, 3u, 64u, 65u}) {
        const SurfaceLayout L = surface_layout(n_frames, n_sectors);
        const uint32_t total = n_frames * n_sectors;
        CHECK(L.cells == total && L.rows == (size_t)total * 8 && L.entries == (size_t)total * 16 && L.side_cap == 64u * n_frames && L.first_bytes >= (n_frames + 1) * 4 &&
              L.table == L.first_bytes + L.side_cap * 24);
        for (uint32_t want_entries : {0u, 1u, 255u, 256u, 257u, total}) {
            const uint32_t n_entries = want_entries < total ? want_entries : total;
            std::vector<std::vector<dg_sector_flats>> given(n_frames);
            std::vector<uint8_t> used(total, 0);
            for (uint32_t e = 0; e < n_entries; e++) {
                uint32_t cell = n_entries == total ? e : rnd(seed) % total;
                while (used[cell]) cell = (cell + 1) % total;
                used[cell] = 1;
                const int32_t s = (int32_t)(cell % n_sectors);
                if (e % 5 == 0) given[cell / n_sectors].push_back(dg_sector_flats{s, f_sky, f_sky});
                given[cell / n_sectors].push_back(dg_sector_flats{s, handles[rnd(seed) % 3], handles[rnd(seed) % 3]});
            }
            std::vector<FlatEntry> staged(L.cells);
            std::vector<FsFlats> want(total);
            uint32_t n_staged = 0;
            for (uint32_t fr = 0; fr < n_frames; fr++) {
                for (uint32_t s = 0; s < n_sectors; s++) want[fr * n_sectors + s] = sc.fs_flats[s];
                for (const dg_sector_flats &g : given[fr]) want[fr * n_sectors + (uint32_t)g.sector] = FsFlats{g.floor_flat, g.ceil_flat};
                const dg_view_surfaces vs{nullptr, 0, given[fr].data(), (uint32_t)given[fr].size()};
                CHECK(resolve_view_surfaces(sc, nullptr, vs, (int32_t)fr, latest_sides, latest_flats) == 0u);
                for (const FlatEntry &g : flats) { CHECK(n_staged < L.cells); staged[n_staged++] = g; }
            }
            CHECK(n_staged == n_entries);
            std::vector<FsFlats> rows(total, FsFlats{-1, -1});
            const FlatRowParams P{sc.fs_flats.data(), staged.data(), rows.data(), n_sectors, n_frames, n_staged};
            for (uint32_t b = 0; b < (total + 255u) / 256u; b++)
                for (uint32_t t = 0; t < 256; t++)
                    if (b * 256u + t < P.n_frames * P.n_items) view_row_fill(P, b * 256u + t);
            for (uint32_t b = 0; b < (n_staged + 255u) / 256u; b++)
                for (uint32_t t = 0; t < 256; t++)
                    if (b * 256u + t < P.n_entries) view_row_scatter(P, b * 256u + t);
            CHECK(std::memcmp(rows.data(), want.data(), (size_t)total * sizeof(FsFlats)) == 0);
            cells_checked += total;
        }
    }
    {   // an entry outside the batch is left alone (the host has checked both; the body checks again)
        std::vector<FsFlats> rows(2 * n_sectors, FsFlats{7, 7});
        const FlatEntry bad[] = {{2, 0, {1, 1}}, {-1, 0, {1, 1}}, {0, (int32_t)n_sectors, {1, 1}}, {0, -1, {1, 1}}, {1, (int32_t)n_sectors - 1, {5, 6}}};
        const FlatRowParams P{sc.fs_flats.data(), bad, rows.data(), n_sectors, 2, 5};
        for (uint32_t e = 0; e < 5; e++) view_row_scatter(P, e);
        for (uint32_t i = 0; i + 1 < 2 * n_sectors; i++) CHECK(rows[i].floor == 7 && rows[i].ceil == 7);
        CHECK(rows[2 * n_sectors - 1].floor == 5 && rows[2 * n_sectors - 1].ceil == 6);
    }
    {   // the handle encoding round trip
        for (int32_t flat : {0, 1, 4095}) CHECK(fs_handle_flat(fs_flat_handle(flat, -1, true)) == flat && fs_handle_anim(fs_flat_handle(flat, -1, false)) == -1);
        for (int32_t anim : {0, 7, 100000}) CHECK(fs_handle_anim(fs_flat_handle(-2, anim, true)) == anim);
        CHECK(fs_handle_flat(fs_flat_handle(-2, -1, false)) == -2 && fs_flat_handle(-2, -1, true) > 0);
    }

    // the host walker with entries, through the C-ABI
    uint64_t renders = 0;
    for (int fr : {40, 323, 640, 817}) {
        dg_view v{};
        const float *r = path.data() + 8 * fr;
        v.x = r[0]; v.y = r[1]; v.angle = r[2]; v.floor_height = r[7]; v.timestamp = 0.4f;
        dg_frame_lists plain{}, fl{};
        CHECK(dg_build_lists(h, 160, 100, &v, &plain) == DG_OK);
        const uint32_t n_plain = plain.n_renders, n_plain_planes = plain.n_visplanes;
        std::vector<dg_side_surface> all;
        std::vector<dg_sector_flats> allf;
        for (uint32_t i = 0; i < n_sides; i += 2) {
            const SidedefRec &d = sc.sidedefs[i];
            all.push_back(dg_side_surface{(int32_t)i, d.middle < 0 ? (rnd(seed) % 4 ? -1 : t_grate) : t_wide, d.lower < 0 ? -1 : t_brick, d.upper < 0 ? -1 : t_wide, (int32_t)(rnd(seed) % 65536) - 32768,
                                          (int32_t)(rnd(seed) % 65536) - 32768});
        }
        for (uint32_t s = 0; s < n_sectors; s++) allf.push_back(dg_sector_flats{(int32_t)s, handles[rnd(seed) % 3], handles[rnd(seed) % 3]});
        const dg_view_surfaces vs{all.data(), (uint32_t)all.size(), allf.data(), (uint32_t)allf.size()};
        const uint32_t *owners = nullptr;
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, &vs, &fl, &owners) == DG_OK);
        renders += fl.n_renders;
        const dg_view_surfaces none{nullptr, 0, nullptr, 0};
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, &none, &fl, nullptr) == DG_OK && fl.n_renders == n_plain && fl.n_visplanes == n_plain_planes);
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, nullptr, &fl, nullptr) == DG_OK && fl.n_renders == n_plain);
        const dg_side_surface wild{(int32_t)n_sides, -1, -1, -1, 0, 0}, far{0, -1, -1, -1, 40000, 0};
        const dg_view_surfaces w{&wild, 1, nullptr, 0}, t{&far, 1, nullptr, 0}, null_arr{nullptr, 2, nullptr, 0};
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, &w, &fl, nullptr) == DG_ERR_INVALID);
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, &t, &fl, nullptr) == DG_ERR_INVALID);
        CHECK(dg_build_lists_surfaces(h, 160, 100, &v, nullptr, nullptr, &null_arr, &fl, nullptr) == DG_ERR_INVALID);
    }
    CHECK(renders > 0 && cells_checked > 0);
    dg_scene_free(h);
    std::printf("surfaces_host_main: ok (%llu cells, %llu renders)\n", (unsigned long long)cells_checked, (unsigned long long)renders);
    return 0;
}
