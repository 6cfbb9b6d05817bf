// floor_map_host.hpp — the host side of the floor-textured player-centred map frames, shared by api_scene.cpp
// (dg_floor_map_host) and context.cpp (dg_submit_floor_map_views): the contract's checks, the scene's tables as the kernels read them,
// a view's row of floor cells, the sector row of a mask, and the frame by the literal rule.  The rule itself is floor_map_core.h's.
#pragma once
#include <string>
#include <vector>

#include "ego_host.hpp"
#include "floor_map_core.h"
#include "frontend.hpp"

namespace dg {

// Per call: ego_check_call, and a scene whose BSP has leaves.
inline int floor_check_call(const Scene &sc, int W, int H, const dg_ego_map *p, std::string &err) {
    const int rc = ego_check_call(sc, W, H, p, err);
    if (rc) return rc;
    if (sc.subsectors.empty() || sc.sectors.empty() || sc.walk_leaf_sector.size() != sc.subsectors.size()) { err = "floor map frames: the scene has no subsectors"; return DG_ERR_INVALID; }
    return DG_OK;
}

// The scene's tables: per leaf its segs and walk_leaf_sector, per seg its two vertices, per linedef the sectors of its two sidedefs.
// A leaf whose seg range leaves the seg table is given no sector (never, for a map the loader accepted).
struct FloorHostTables {
    std::vector<FloorLeaf> leaves;
    std::vector<FloorSeg> segs;
    std::vector<FloorLine> lines;
};
inline void floor_tables(const Scene &sc, FloorHostTables &t) {
    const size_t n_segs = sc.segs.size();
    t.leaves.resize(sc.subsectors.size());
    for (size_t l = 0; l < t.leaves.size(); l++) {
        const SubSectorRec &ss = sc.subsectors[l];
        const bool ok = ss.first >= 0 && ss.count >= 0 && (size_t)ss.first <= n_segs && (size_t)ss.count <= n_segs - (size_t)ss.first;
        t.leaves[l] = ok ? FloorLeaf{(uint32_t)ss.first, (uint32_t)ss.count, sc.walk_leaf_sector[l]} : FloorLeaf{0u, 0u, -1};
    }
    t.segs.resize(n_segs);
    for (size_t k = 0; k < n_segs; k++) {
        const SegRec &sg = sc.segs[k];
        t.segs[k] = FloorSeg{sc.vx[(size_t)sg.v1], sc.vy[(size_t)sg.v1], sc.vx[(size_t)sg.v2], sc.vy[(size_t)sg.v2]};
    }
    t.lines.resize(sc.linedefs.size());
    for (size_t k = 0; k < t.lines.size(); k++) {
        const LinedefRec &d = sc.linedefs[k];
        const auto sector = [&](int32_t sd) { return sd >= 0 && (size_t)sd < sc.sidedefs.size() ? sc.sidedefs[(size_t)sd].sector : -1; };
        t.lines[k] = FloorLine{sector(d.front), sector(d.back)};
    }
}
// ... as floor_map_core.h reads them on the host.
inline FloorTables floor_tables_host(const Scene &sc, const FloorHostTables &t, const uint32_t *palette) {
    return FloorTables{sc.walk_nodes.data(), (uint32_t)sc.walk_nodes.size(), t.leaves.data(), (uint32_t)t.leaves.size(), t.segs.data(), (uint32_t)t.segs.size(),
                       sc.flat_pool.data(), (uint32_t)(sc.flat_pool.size() / 4096u), palette, (uint32_t)sc.sectors.size()};
}
inline void floor_palette(const Scene &sc, uint32_t pal[256]) {
    for (int i = 0; i < 256; i++) pal[i] = (uint32_t)sc.palette[3 * i] | ((uint32_t)sc.palette[3 * i + 1] << 8) | ((uint32_t)sc.palette[3 * i + 2] << 16);
}

// What a view's row is built with, kept from one view to the next.
struct FloorRowScratch {
    std::vector<int32_t> handle;        // per sector: the view's floor flat handle
    std::vector<int32_t> light;         // ... and its light level
    LatestSides sides;
    LatestFlats flats;
};

// One view's cells [sectors] (trig and timestamp as the view has them).  The flat: a dg_sector_flats entry of the view, else the
// scene's; the light: a dg_sector_light entry of the view, else the light effect's level at the timestamp (lfx: the effects drawn
// with, or null), else the scene's.  Only state->lights and surfaces->flats are read; the flats entries are validated as
// resolve_view_surfaces validates them.  DG_ERR_INVALID with err for an entry out of range; the row is then not to be used.
inline int floor_view_cells(const Scene &sc, const LightFx *lfx, const dg_view &view, const dg_view_state *state, const dg_view_surfaces *surfaces,
                            FloorRowScratch &A, FloorCell *row, std::string &err) {
    const size_t S = sc.sectors.size();
    A.handle.resize(S); A.light.resize(S);
    for (size_t s = 0; s < S; s++) { A.handle[s] = sc.fs_flats[s].floor; A.light[s] = sc.sectors[s].light; }
    if (lfx && lfx->fits(sc))
        for (size_t r = 0; r < lfx->recs.size(); r++) A.light[(size_t)lfx->recs[r].sector] = lfx->level(r, view.timestamp);
    if (surfaces) {
        const dg_view_surfaces only{nullptr, 0u, surfaces->flats, surfaces->n_flats};
        const unsigned bad = resolve_view_surfaces(sc, nullptr, only, 0, A.sides, A.flats);
        if (bad) { err = view_surfaces_error(bad); return DG_ERR_INVALID; }
        for (const FlatEntry &e : A.flats.out) A.handle[(size_t)e.sector] = e.flats.floor;
    }
    if (state) {
        if (state->n_lights && !state->lights) { err = "view state with a null array"; return DG_ERR_INVALID; }
        const dg_view_state only{state->lights, state->n_lights, nullptr, 0u};
        const unsigned bad = apply_view_state(sc, only, [&](size_t k, int32_t level) { A.light[k] = level; }, [](size_t, int32_t) {});
        if (bad) { err = "view state: sector index out of range"; return DG_ERR_INVALID; }
    }
    const uint32_t n_flats = (uint32_t)(sc.flat_pool.size() / 4096u);
    for (size_t s = 0; s < S; s++) row[s] = floor_cell(A.handle[s], sc.fs_anims.data(), (uint32_t)sc.fs_anims.size(), n_flats, view.timestamp, (int16_t)A.light[s]);
    return DG_OK;
}

inline size_t floor_seen_words(const Scene &sc) { return (sc.sectors.size() + 31u) / 32u; }
// The sector row of a mask row: what dg_floor_seen_sectors builds on the GPU.
inline void floor_seen_row(const Scene &sc, const FloorHostTables &t, const uint32_t *mask_row, uint32_t *seen) {
    std::fill(seen, seen + floor_seen_words(sc), 0u);
    for (size_t l = 0; l < t.lines.size(); l++) {
        if (!floor_seen_line(mask_row, (uint32_t)l)) continue;
        for (const int32_t s : {t.lines[l].front, t.lines[l].back})
            if (s >= 0 && (size_t)s < sc.sectors.size()) seen[(size_t)s >> 5] |= 1u << ((uint32_t)s & 31u);
    }
}

// What the floor under one view's frame is drawn with on the host: the scene's tables, the view's cells and its sector row.
struct FloorFrameHost {
    FloorHostTables t;
    FloorRowScratch A;
    std::vector<FloorCell> row;
    std::vector<uint32_t> seen;
    uint32_t pal[256];
};
// ... built, with every check of the view's state and surfaces (floor_view_cells).
inline int floor_frame_prepare(const Scene &sc, const LightFx *lfx, const dg_view &view, const uint32_t *mask_row, const dg_view_state *state,
                               const dg_view_surfaces *surfaces, FloorFrameHost &F, std::string &err) {
    floor_tables(sc, F.t);
    F.row.resize(sc.sectors.size());
    const int rc = floor_view_cells(sc, lfx, view, state, surfaces, F.A, F.row.data(), err);
    if (rc) return rc;
    F.seen.clear();
    if (mask_row) { F.seen.resize(floor_seen_words(sc)); floor_seen_row(sc, F.t, mask_row, F.seen.data()); }
    floor_palette(sc, F.pal);
    return DG_OK;
}
// Every pixel of the frame that no line covers (covered(Y * W + X) false) through floor_pixel.
template <class Covered>
inline void floor_frame_fill(const Scene &sc, const FloorFrameHost &F, int W, int H, const dg_view &view, const dg_ego_map &p, const uint32_t *mask_row, uint8_t *out,
                             Covered covered) {
    const FloorTables T = floor_tables_host(sc, F.t, F.pal);
    const EgoView v = ego_view(view);
    const float inv = 1.0f / p.scale;
    const bool rotate = (p.flags & EGO_ROTATE) != 0;
    for (int32_t Y = 0; Y < H; Y++)
        for (int32_t X = 0; X < W; X++) {
            const size_t at = (size_t)Y * (size_t)W + (size_t)X;
            if (covered(at)) continue;
            uint8_t *const px = out + 3 * at;
            const uint32_t c = floor_value_rgb(floor_pixel(T, F.row.data(), mask_row ? F.seen.data() : nullptr, X, Y, W, H, v, inv, rotate));
            px[0] = (uint8_t)c; px[1] = (uint8_t)(c >> 8); px[2] = (uint8_t)(c >> 16);
        }
}

// One frame by the literal rule (call and view checked, trig filled): dg_ego_map_host's frame, and every pixel it left black through
// floor_pixel.  (A line is never black: red or yellow.)
inline int floor_frame_host(const Scene &sc, const LightFx *lfx, int W, int H, const dg_view &view, const dg_ego_map &p, const uint32_t *mask_row,
                            const dg_view_state *state, const dg_view_surfaces *surfaces, uint8_t *out, std::string &err) {
    std::vector<dg_map_line> lines;
    int rc = ego_frame_lines(sc, W, H, view, p, mask_row, lines, err);
    if (rc) return rc;
    FloorFrameHost F;
    rc = floor_frame_prepare(sc, lfx, view, mask_row, state, surfaces, F, err);
    if (rc) return rc;
    map_draw_lines_host(lines.data(), lines.size(), W, H, out, [](size_t) { return true; });
    floor_frame_fill(sc, F, W, H, view, p, mask_row, out, [&](size_t at) { return (out[3 * at] | out[3 * at + 1] | out[3 * at + 2]) != 0; });
    return DG_OK;
}

}  // namespace dg
