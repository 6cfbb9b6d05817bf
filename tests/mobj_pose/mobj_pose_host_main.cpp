// tests/mobj_pose/mobj_pose_host_main.cpp — the per-view map-object poses' host side as a stand-alone program, for a sanitizer build
// (tests/test_mobj_pose_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
//   usage: mobj_pose_host_main <wad file> <camera path .f32> <map name>
// view_rows_core.h's fill and scatter bodies run lane after lane for the pose kind (mobj_pose_core.h), as the two kernels index them (256-lane groups, the last one partial),
// over batches and entry counts at the kernels' boundaries; every row is compared with Scene::sector_from_vertex.  Then the host walker
// with poses through the C-ABI: the lists of dg_build_lists_poses against the rows.  It checks what it gets.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <string>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/api_common.hpp"
#include "../../doom-rust-renderer_amd/csrc/frontend.hpp"
#include "../../doom-rust-renderer_amd/csrc/mobj_pose_core.h"

using namespace dg;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("mobj_pose_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rnd(uint32_t &s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// The points a pose may name: inside the map, far outside, on and next to partition lines, on vertices, NaN and infinities.
static std::vector<V2> points(const Scene &sc) {
    std::vector<V2> p;
    uint32_t s = 2463534242u;
    for (int i = 0; i < 300; i++) p.push_back(V2{(float)(rnd(s) % 4500) - 200.0f + 0.25f * (float)(rnd(s) % 4), (float)(rnd(s) % 3500) - 200.0f});
    for (int i = 0; i < 60; i++) p.push_back(V2{(float)(int)(rnd(s) % 60000) - 30000.0f, (float)(int)(rnd(s) % 60000) - 30000.0f});
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (const WalkNode &n : sc.walk_nodes)
        for (float t : {0.0f, 0.5f, 1.0f, -0.75f, 1.0f / 3.0f}) {
            const float x = n.x + t * n.dx, y = n.y + t * n.dy;
            p.push_back(V2{x, y});
            p.push_back(V2{std::nextafterf(x, inf), y});
            p.push_back(V2{x, std::nextafterf(y, -inf)});
        }
    for (size_t i = 0; i < sc.vx.size(); i++) p.push_back(V2{sc.vx[i], sc.vy[i]});
    const float odd[] = {nan, inf, -inf, 0.0f, 1000.0f, 3.0e38f};
    for (float a : odd)
        for (float b : odd) p.push_back(V2{a, b});
    return p;
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
    const uint32_t n_mobjs = (uint32_t)sc.mobjs.size();
    CHECK(n_mobjs > 0 && !sc.walk_nodes.empty() && sc.walk_leaf_sector.size() == sc.subsectors.size());
    const std::vector<V2> pts = points(sc);

    // the leaf table against the host rule, and the two host-only calls
    uint64_t none = 0;
    {
        std::vector<float> xs, ys;
        for (const V2 &p : pts) { xs.push_back(p.x); ys.push_back(p.y); }
        std::vector<int32_t> got(pts.size(), 12345);
        CHECK(dg_scene_sectors_at(h, xs.data(), ys.data(), (int)pts.size(), got.data()) == DG_OK);
        for (size_t i = 0; i < pts.size(); i++) {
            const int32_t want = sc.sector_from_vertex(pts[i].x, pts[i].y);
            CHECK(got[i] == want);
            CHECK(pose_sector_at(sc.walk_nodes.data(), (int32_t)sc.walk_nodes.size() - 1, sc.walk_leaf_sector.data(), pts[i].x, pts[i].y) == want);
            CHECK(want >= -1 && want < (int32_t)sc.sectors.size());
            none += want < 0;
        }
        std::vector<dg_mobj_placed> placed(n_mobjs);
        CHECK(dg_scene_mobj_poses(h, placed.data(), (int)n_mobjs) == DG_OK);
        CHECK(dg_scene_mobj_poses(h, placed.data(), (int)n_mobjs + 1) == DG_ERR_INVALID);
        for (uint32_t m = 0; m < n_mobjs; m++) CHECK(std::memcmp(&placed[m], &sc.fs_mobjs[m], sizeof(FsMobj)) == 0);
    }

    // the bodies, lane after lane
    const uint32_t batches[] = {1, 3, 64, 65};
    uint64_t rows_checked = 0, placed_rows = 0;
    uint32_t s = 88172645u;
    for (uint32_t n_frames : batches) {
        const uint32_t cells = n_frames * n_mobjs;
        const uint32_t totals[] = {0, 1, 63, 64, 65, 255, 256, 257, cells};
        for (uint32_t want_entries : totals) {
            const uint32_t n_entries = want_entries < cells ? want_entries : cells;
            // unique (frame, object) pairs: a stride walk over the cells (the stride is coprime to their number)
            uint32_t stride = 1 + rnd(s) % (cells ? cells : 1);
            auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
            while (gcd(stride, cells) != 1) stride++;
            std::vector<PoseEntry> entries(n_entries);
            for (uint32_t e = 0; e < n_entries; e++) {
                const uint32_t cell = (uint32_t)(((uint64_t)e * stride + 5) % cells);
                const V2 p = pts[rnd(s) % pts.size()];
                entries[e] = PoseEntry{(int32_t)(cell / n_mobjs), (int32_t)(cell % n_mobjs), p.x, p.y, (float)(rnd(s) % 6283) / 1000.0f - 3.1f};
            }
            std::vector<FsMobj> rows(cells, FsMobj{-1.0f, -1.0f, -1.0f, -7});
            PoseParams P{};
            P.scene_rows = sc.fs_mobjs.data(); P.ctx.nodes = sc.walk_nodes.data(); P.ctx.leaf_sector = sc.walk_leaf_sector.data();
            P.entries = entries.data(); P.rows = rows.data();
            P.ctx.root = (int32_t)sc.walk_nodes.size() - 1;
            P.n_items = n_mobjs; P.n_frames = n_frames; P.n_entries = n_entries;
            for (uint32_t g = 0; g < (cells + 255u) / 256u; g++)              // dg_mobj_pose_fill
                for (uint32_t t = 0; t < 256u; t++) {
                    const uint32_t idx = g * 256u + t;
                    if (idx >= P.n_frames * P.n_items) continue;
                    view_row_fill(P, idx);
                }
            for (uint32_t g = 0; g < (n_entries + 255u) / 256u; g++)          // dg_mobj_pose_place
                for (uint32_t t = 0; t < 256u; t++) {
                    const uint32_t e = g * 256u + t;
                    if (e >= P.n_entries) continue;
                    view_row_scatter(P, e);
                }
            std::vector<int32_t> entry_of(cells, -1);
            for (uint32_t e = 0; e < n_entries; e++) {
                int32_t &at = entry_of[(size_t)entries[e].frame * n_mobjs + (uint32_t)entries[e].mobj];
                CHECK(at < 0);                                               // (unique)
                at = (int32_t)e;
            }
            for (uint32_t c = 0; c < cells; c++) {
                const FsMobj &r = rows[c];
                if (entry_of[c] < 0) { CHECK(std::memcmp(&r, &sc.fs_mobjs[c % n_mobjs], sizeof(FsMobj)) == 0); }
                else {
                    const PoseEntry &en = entries[(size_t)entry_of[c]];
                    CHECK(same_bits(r.x, en.x) && same_bits(r.y, en.y) && same_bits(r.angle, en.angle));
                    CHECK(r.sector == sc.sector_from_vertex(en.x, en.y));
                    placed_rows++;
                }
                rows_checked++;
            }
        }
    }

    // the host walker with poses: the later of two entries wins, an index out of range is refused, the loaded pose changes nothing
    uint64_t frames = 0, changed = 0;
    for (int i = 0; i < 1000; i += 91) {
        const float *r = &path[(size_t)i * 8];
        const dg_view v{r[0], r[1], r[2], r[7], r[3], r[4], r[5], r[6], 0.0f, 1};
        dg_frame_lists fl;
        CHECK(dg_build_lists(h, 160, 100, &v, &fl) == DG_OK);
        const std::vector<dg_bitmap_render> plain(fl.renders, fl.renders + fl.n_renders);
        std::vector<dg_mobj_pose> ps;
        for (uint32_t m = 0; m < n_mobjs; m++) ps.push_back(dg_mobj_pose{(int32_t)m, sc.mobjs[m].x, sc.mobjs[m].y, sc.mobjs[m].angle});
        dg_view_poses vp{ps.data(), (uint32_t)ps.size()};
        const uint32_t *owners = nullptr;
        CHECK(dg_build_lists_poses(h, 160, 100, &v, &vp, &fl, &owners) == DG_OK);
        CHECK(fl.n_renders == plain.size() && (plain.empty() || std::memcmp(fl.renders, plain.data(), plain.size() * sizeof(dg_bitmap_render)) == 0));
        // every object a few frames ahead of the camera, each entry preceded by one that loses
        ps.clear();
        for (uint32_t m = 0; m < n_mobjs; m++) {
            const float *t = &path[(size_t)((i + 5 + 3 * (int)m) % 1000) * 8];
            ps.push_back(dg_mobj_pose{(int32_t)m, std::numeric_limits<float>::quiet_NaN(), 3.0e38f, 1.0f});
            ps.push_back(dg_mobj_pose{(int32_t)m, std::floor(t[0]) + 0.5f, std::floor(t[1]) - 0.25f, 0.1f * (float)m});
        }
        vp = dg_view_poses{ps.data(), (uint32_t)ps.size()};
        CHECK(dg_build_lists_poses(h, 160, 100, &v, &vp, &fl, &owners) == DG_OK);
        changed += fl.n_renders != plain.size() || (!plain.empty() && std::memcmp(fl.renders, plain.data(), plain.size() * sizeof(dg_bitmap_render)) != 0);
        for (uint32_t k = 0; k < fl.n_renders; k++)
            if ((owners[k] >> 16) == DG_LABEL_MOBJ) CHECK((owners[k] & 0xffffu) < n_mobjs);
        ps.push_back(dg_mobj_pose{(int32_t)n_mobjs, 0.0f, 0.0f, 0.0f});
        vp = dg_view_poses{ps.data(), (uint32_t)ps.size()};
        CHECK(dg_build_lists_poses(h, 160, 100, &v, &vp, &fl, nullptr) == DG_ERR_INVALID);
        CHECK(std::string(dg_last_error()).find("map object index out of range") != std::string::npos);
        CHECK(dg_build_lists(h, 160, 100, &v, &fl) == DG_OK);                  // (the refused call left the arena's rows clean)
        CHECK(fl.n_renders == plain.size() && (plain.empty() || std::memcmp(fl.renders, plain.data(), plain.size() * sizeof(dg_bitmap_render)) == 0));
        frames++;
    }
    CHECK(placed_rows > 1000 && changed > frames / 2);
    dg_scene_free(h);
    std::printf("mobj_pose_host_main: ok (%llu rows, %llu placed, %llu points in no sector, %llu frames, %llu changed)\n", (unsigned long long)rows_checked,
                (unsigned long long)placed_rows, (unsigned long long)none, (unsigned long long)frames, (unsigned long long)changed);
    return 0;
}
