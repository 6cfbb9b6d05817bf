// map_things_host.hpp — the host side of the map-object markers on the map frames, shared by api_scene.cpp
// (dg_scene_set_map_markers, dg_map_thing_lines, dg_ego_map_things_host, dg_floor_map_things_host) and context.cpp
// (dg_submit_ego_map_views_things, dg_submit_floor_map_views_things): the checks, the scene's tables as the kernels read them, a view's
// shown bits and sorted pose entries, and the frames by the literal rule.  The rules themselves are map_things_core.h's.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "floor_map_host.hpp"
#include "map_things_core.h"

namespace dg {

// dg_scene_set_map_markers' checks of a table for a scene with n_mobjs map objects.
inline int thing_check_markers(const dg_map_marker *markers, int n, size_t n_mobjs, std::string &err) {
    if (!markers && n == 0) return DG_OK;
    if (!markers) { err = "map markers: null table"; return DG_ERR_INVALID; }
    if (n < 0 || (size_t)n != n_mobjs) { err = "map markers: n must equal dg_scene_mobj_count"; return DG_ERR_INVALID; }
    for (int i = 0; i < n; i++) {
        const dg_map_marker &m = markers[i];
        if (m.radius < 0 || m.radius > THING_MAX_RADIUS) { err = "map markers: radius outside [0, 1024]"; return DG_ERR_INVALID; }
        if (m.rgb > 0xffffffu) { err = "map markers: rgb above 0xffffff"; return DG_ERR_INVALID; }
        if (m.flags & ~(MARK_BOX | MARK_HEADING)) { err = "map markers: unknown flag bits"; return DG_ERR_INVALID; }
    }
    return DG_OK;
}

// Per call of the thing functions: the scene's object count.
inline int thing_check_call(const Scene &sc, std::string &err) {
    if (sc.mobjs.size() > THING_MAX) { err = "map markers: more than 65536 map objects"; return DG_ERR_CAPACITY; }
    return DG_OK;
}

// The marker table the functions draw with: the given one if it fits the scene (a table set before the scene's objects changed does
// not: no markers).
inline const std::vector<dg_map_marker> *thing_markers(const Scene &sc, const std::vector<dg_map_marker> &markers) {
    return !markers.empty() && markers.size() == sc.mobjs.size() ? &markers : nullptr;
}

// The tables as the kernels read them: per object its marker and its place as loaded (cosf / sinf of the angle from the host's libm).
inline void thing_tables(const Scene &sc, const std::vector<dg_map_marker> &markers, std::vector<ThingMarker> &tm, std::vector<ThingPlace> &tp) {
    const size_t n = sc.mobjs.size();
    tm.resize(n); tp.resize(n);
    for (size_t i = 0; i < n; i++) {
        tm[i] = ThingMarker{(float)markers[i].radius, markers[i].rgb, markers[i].flags};
        tp[i] = ThingPlace{sc.mobjs[i].x, sc.mobjs[i].y, cosf(sc.mobjs[i].angle), sinf(sc.mobjs[i].angle)};
    }
}

// What a view's row and entries are built with, kept from one view to the next.
struct ThingViewScratch {
    std::vector<int32_t> state;         // per object: mfx_encode of the state the view shows it in
    LatestPoses poses;
};

// One view's shown bits (row: thing_shown_words words, written whole) and its pose entries after later-wins, sorted by object, appended
// to `entries` — only those of shown objects: nothing else reads one.  The state composes as for the colour frame: a dg_view_state entry
// wins, else the thinker's (mfx: the thinkers drawn with, or null), else the scene's.  state / poses are validated as the view
// submissions validate them.  DG_ERR_INVALID with err; row and entries are then not to be used.
inline int thing_view_rows(const Scene &sc, const std::vector<dg_map_marker> &markers, const MobjFx *mfx, const dg_view &view, const dg_view_state *state,
                           const dg_view_poses *poses, ThingViewScratch &A, uint32_t *row, std::vector<ThingEntry> &entries, std::string &err) {
    const size_t n = sc.mobjs.size();
    if (!check_view_inputs(ViewInputs{state, poses}, err)) return DG_ERR_INVALID;
    A.state.resize(n);
    for (size_t i = 0; i < n; i++) A.state[i] = mfx_encode(sc.mobjs[i].sprite_frame, sc.mobjs[i].full_bright);
    if (mfx && mfx->fits(sc))
        for (uint32_t i : mfx->driven) A.state[i] = mfx->value(i, view.timestamp);
    if (state) {
        const unsigned bad = apply_view_state(sc, *state, [](size_t, int32_t) {}, [&](size_t i, int32_t val) { A.state[i] = val; });
        if (bad) { err = bad & 2u ? "view state: map object or sprite frame index out of range" : "view state: sector index out of range"; return DG_ERR_INVALID; }
    }
    const bool moved = poses != nullptr;
    if (moved && !resolve_view_poses(sc, *poses, A.poses)) {
        A.poses.release();
        err = "view poses: map object index out of range";
        return DG_ERR_INVALID;
    }
    std::fill(row, row + thing_shown_words((uint32_t)n), 0u);
    for (size_t i = 0; i < n; i++) {
        if (markers[i].flags == 0u || A.state[i] < 0) continue;
        const int32_t at = moved ? A.poses.of[i] : -1;
        const float x = at < 0 ? sc.mobjs[i].x : A.poses.out[(size_t)at].x, y = at < 0 ? sc.mobjs[i].y : A.poses.out[(size_t)at].y;
        if (!thing_position_ok(x, y)) continue;
        row[i >> 5] |= 1u << (i & 31u);
        if (at >= 0) entries.push_back(ThingEntry{(int32_t)i, x, y, cosf(A.poses.out[(size_t)at].angle), sinf(A.poses.out[(size_t)at].angle)});   // (in object order: sorted)
    }
    if (moved) A.poses.release();
    return DG_OK;
}

// The marker lines of one frame in draw order from its row and entries (view checked, trig filled): transformed, unclipped.
inline void thing_frame_lines(const Scene &sc, int W, int H, const dg_view &view, const dg_ego_map &p, const ThingMarker *tm, const ThingPlace *tp, const uint32_t *row,
                              const ThingEntry *entries, uint32_t n_entries, std::vector<dg_map_line> &out) {
    const EgoView v = ego_view(view);
    const bool rotate = (p.flags & EGO_ROTATE) != 0;
    for (uint32_t i = 0; i < (uint32_t)sc.mobjs.size(); i++) {
        if (!thing_shown(row, i)) continue;
        const ThingPlace place = thing_place(entries, n_entries, tp, i);
        for (uint32_t e = 0; e < THING_EDGES; e++) {
            EgoLine m;
            if (!thing_edge(place, tm[i], e, m)) continue;
            dg_map_line l;
            ego_point(m.x0, m.y0, v, p.scale, rotate, W, H, l.x0, l.y0);
            ego_point(m.x1, m.y1, v, p.scale, rotate, W, H, l.x1, l.y1);
            l.rgb = tm[i].rgb;
            out.push_back(l);
        }
    }
}

// ... of a view with its state and poses (markers: thing_markers' table, or null: none).
inline int thing_view_lines(const Scene &sc, const std::vector<dg_map_marker> *markers, const MobjFx *mfx, int W, int H, const dg_view &view, const dg_ego_map &p,
                            const dg_view_state *state, const dg_view_poses *poses, std::vector<dg_map_line> &out, std::string &err) {
    if (!markers) return check_view_inputs(ViewInputs{state, poses}, err) ? DG_OK : DG_ERR_INVALID;
    std::vector<ThingMarker> tm;
    std::vector<ThingPlace> tp;
    thing_tables(sc, *markers, tm, tp);
    ThingViewScratch A;
    std::vector<uint32_t> row(thing_shown_words((uint32_t)sc.mobjs.size()));
    std::vector<ThingEntry> entries;
    const int rc = thing_view_rows(sc, *markers, mfx, view, state, poses, A, row.data(), entries, err);
    if (rc) return rc;
    thing_frame_lines(sc, W, H, view, p, tm.data(), tp.data(), row.data(), entries.data(), (uint32_t)entries.size(), out);
    return DG_OK;
}

// The lines of one frame with markers in draw order (view checked, trig filled): the linedefs (ego_frame_lines without the arrow), the
// marker lines, then the arrow's three if the flags ask for it.
inline int thing_all_lines(const Scene &sc, const std::vector<dg_map_marker> *markers, const MobjFx *mfx, int W, int H, const dg_view &view, const dg_ego_map &p,
                           const uint32_t *mask_row, const dg_view_state *state, const dg_view_poses *poses, std::vector<dg_map_line> &out, std::string &err) {
    const dg_ego_map plain{p.scale, p.flags & ~EGO_ARROW};
    int rc = ego_frame_lines(sc, W, H, view, plain, mask_row, out, err);
    if (!rc) rc = thing_view_lines(sc, markers, mfx, W, H, view, p, state, poses, out, err);
    if (rc || !(p.flags & EGO_ARROW)) return rc;
    dg_map_line arrow[3];
    rc = ego_arrow_lines(W, H, view, p, arrow, err);
    if (!rc) out.insert(out.end(), arrow, arrow + 3);
    return rc;
}

// The lines drawn in order point by point (map_draw_lines_host), and which pixels any of them wrote.
inline void thing_draw_lines_host(const std::vector<dg_map_line> &lines, int32_t W, int32_t H, uint8_t *rgb24, std::vector<uint8_t> *covered) {
    map_draw_lines_host(lines.data(), lines.size(), W, H, rgb24, [](size_t) { return true; });
    if (!covered) return;
    covered->assign((size_t)W * (size_t)H, 0);
    for (const dg_map_line &l : lines) {
        const MapSeg sg = map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
        for (int32_t i = 0; i < sg.count; i++) {
            int32_t x, y;
            map_seg_point(sg, (int64_t)sg.first + i, x, y);
            if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) (*covered)[(size_t)y * (size_t)W + (size_t)x] = 1;
        }
    }
}

}  // namespace dg
