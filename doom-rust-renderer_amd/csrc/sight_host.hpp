// sight_host.hpp — the host side of the line-of-sight queries, shared by api_scene.cpp (dg_sight_host,
// dg_sight_mobjs_host) and api_device.cpp (dg_sight_device, dg_sight_mobjs_device): the calls' checks, the scene's tables as the
// traversal reads them, a batch's height and pose rows from its entries, and the host twin.  The rule itself is sight_core.h's.
#pragma once
#include <string>
#include <vector>

#include "floor_map_host.hpp"
#include "frontend.hpp"
#include "mobj_pose_core.h"
#include "sight_core.h"

namespace dg {

// The scene's tables: per leaf its segs, per seg its linedef, per linedef its vertices, its sidedefs' sectors and its flags.
struct SightHostTables {
    std::vector<FloorLeaf> leaves;
    std::vector<uint32_t> seg_line;
    std::vector<SightLine> lines;
};
inline void sight_tables(const Scene &sc, SightHostTables &t) {
    FloorHostTables f;
    floor_tables(sc, f);
    t.leaves = std::move(f.leaves);
    t.seg_line.resize(sc.segs.size());
    for (size_t k = 0; k < sc.segs.size(); k++) t.seg_line[k] = (uint32_t)sc.segs[k].linedef;
    t.lines.resize(sc.linedefs.size());
    for (size_t k = 0; k < t.lines.size(); k++) {
        const LinedefRec &d = sc.linedefs[k];
        t.lines[k] = SightLine{sc.vx[(size_t)d.v1], sc.vy[(size_t)d.v1], sc.vx[(size_t)d.v2], sc.vy[(size_t)d.v2], f.lines[k].front, f.lines[k].back,
                               (uint32_t)(uint16_t)d.flags, 0u};
    }
}
// ... as sight_core.h reads them on the host, over `rows` [row_frames][sectors].
inline SightTables sight_tables_host(const Scene &sc, const SightHostTables &t, const FsHeights *rows, uint32_t row_frames) {
    return SightTables{sc.walk_nodes.data(), (uint32_t)sc.walk_nodes.size(), t.leaves.data(), (uint32_t)t.leaves.size(), t.seg_line.data(), (uint32_t)t.seg_line.size(),
                       t.lines.data(), (uint32_t)t.lines.size(), rows, (uint32_t)sc.sectors.size(), row_frames};
}

inline uint32_t sight_scene_depth(const Scene &sc) {
    std::vector<uint32_t> depth(sc.walk_nodes.size());
    return sight_depth(sc.walk_nodes.data(), (uint32_t)sc.walk_nodes.size(), depth.data());
}
inline size_t sight_words(const Scene &sc) { return (sc.mobjs.size() + 31u) / 32u; }

// A batch's sector entries as the row kernels take them: every frame's entries after later-wins, tagged with the frame.  DG_ERR_INVALID
// with err for a null array or an entry out of range.
inline int sight_sector_entries(const Scene &sc, const dg_view_sectors *sectors, int n_frames, LatestHeights &latest, std::vector<SectorEntry> &out, std::string &err) {
    out.clear();
    if (!sectors) return DG_OK;
    for (int f = 0; f < n_frames; f++) {
        if (sectors[f].n && !sectors[f].heights) { err = "view sectors with a null array (frame " + std::to_string(f) + ")"; return DG_ERR_INVALID; }
        const unsigned bad = resolve_view_sectors(sc, sectors[f], latest);
        latest.release();
        if (bad) { err = std::string(view_sectors_error(bad)) + " (frame " + std::to_string(f) + ")"; return DG_ERR_INVALID; }
        for (const dg_sector_heights &h : latest.out) out.push_back(SectorEntry{f, h.sector, (int16_t)h.floor_height, (int16_t)h.ceiling_height});
    }
    return DG_OK;
}
// ... and its pose entries.
inline int sight_pose_entries(const Scene &sc, const dg_view_poses *poses, int n_frames, LatestPoses &latest, std::vector<PoseEntry> &out, std::string &err) {
    out.clear();
    if (!poses) return DG_OK;
    for (int f = 0; f < n_frames; f++) {
        if (poses[f].n && !poses[f].poses) { err = "view poses with a null array (frame " + std::to_string(f) + ")"; return DG_ERR_INVALID; }
        const bool ok = resolve_view_poses(sc, poses[f], latest);
        latest.release();
        if (!ok) { err = "view poses: map object index out of range (frame " + std::to_string(f) + ")"; return DG_ERR_INVALID; }
        for (const dg_mobj_pose &p : latest.out) out.push_back(PoseEntry{f, p.mobj, p.x, p.y, p.angle});
    }
    return DG_OK;
}

// The height rows of a batch on the host, as HeightRows builds them: no entries: the scene's one row; else [n_frames][sectors].
inline uint32_t sight_height_rows(const Scene &sc, const std::vector<SectorEntry> &entries, int n_frames, std::vector<FsHeights> &rows) {
    const size_t S = sc.sectors.size();
    if (entries.empty()) { rows = sc.fs_heights; return 1u; }
    rows.resize((size_t)n_frames * S);
    SectorRowParams P{sc.fs_heights.data(), entries.data(), rows.data(), (uint32_t)S, (uint32_t)n_frames, (uint32_t)entries.size()};
    for (size_t i = 0; i < rows.size(); i++) view_row_fill(P, (uint32_t)i);
    for (size_t e = 0; e < entries.size(); e++) view_row_scatter(P, (uint32_t)e);
    return (uint32_t)n_frames;
}
// ... and its pose rows, as PoseRows builds them: no entries: the scene's one row (returns 1); else [n_frames][map objects].
inline uint32_t sight_pose_rows(const Scene &sc, const std::vector<PoseEntry> &entries, int n_frames, std::vector<FsMobj> &rows) {
    const size_t M = sc.mobjs.size();
    if (entries.empty()) { rows = sc.fs_mobjs; return 1u; }
    rows.resize((size_t)n_frames * M);
    PoseParams P{sc.fs_mobjs.data(), entries.data(), rows.data(), (uint32_t)M, (uint32_t)n_frames, (uint32_t)entries.size(),
                 PoseCtx{sc.walk_nodes.data(), sc.walk_leaf_sector.data(), (int32_t)sc.walk_nodes.size() - 1}};
    for (size_t i = 0; i < rows.size(); i++) view_row_fill(P, (uint32_t)i);
    for (size_t e = 0; e < entries.size(); e++) view_row_scatter(P, (uint32_t)e);
    return (uint32_t)n_frames;
}

// What dg_sight_host and dg_sight_device check alike, before the entries are looked at.
inline int sight_check_queries(const Scene *sc, int n_frames, const dg_sight_query *q, int n, const uint8_t *out, std::string &err) {
    if (!sc) { err = "null scene"; return DG_ERR_INVALID; }
    if (n < 0 || n_frames < 0) { err = "n and n_frames must not be negative"; return DG_ERR_INVALID; }
    if (n > 0 && (!q || !out)) { err = "null argument"; return DG_ERR_INVALID; }
    if ((uint32_t)n > SIGHT_MAX_QUERIES) { err = "more than 1 << 20 sight queries in one call"; return DG_ERR_CAPACITY; }
    for (int i = 0; i < n; i++)
        if (q[i].frame < 0 || q[i].frame >= n_frames) { err = "sight query " + std::to_string(i) + ": frame outside [0, n_frames)"; return DG_ERR_INVALID; }
    return DG_OK;
}
// ... and the two mobjs calls (M: the scene's map objects).
inline int sight_check_mobjs(const Scene *sc, const dg_view *views, int n, const float *mobj_height, const uint32_t *out, std::string &err) {
    if (!sc) { err = "null scene"; return DG_ERR_INVALID; }
    if (n < 0) { err = "n must not be negative"; return DG_ERR_INVALID; }
    if (n > 0 && (!views || (!sc->mobjs.empty() && (!mobj_height || !out)))) { err = "null argument"; return DG_ERR_INVALID; }
    return DG_OK;
}
inline void sight_views(const dg_view *views, int n, float eye_height, std::vector<SightView> &out) {
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) out[(size_t)i] = SightView{views[i].x, views[i].y, views[i].floor_height + eye_height, 0.0f};
}

// The host twin's stack: as deep as the scene is.
struct SightHostStack {
    std::vector<int32_t> v;
    bool push(int32_t child) { v.push_back(child); return true; }
    bool pop(int32_t &child) {
        if (v.empty()) return false;
        child = v.back();
        v.pop_back();
        return true;
    }
};

}  // namespace dg
