// ego_host.hpp — the host side of the player-centred map frames, shared by api_scene.cpp (dg_ego_map_lines,
// dg_ego_map_host) and context.cpp (dg_submit_ego_map_views): the contract's checks, the arrow's three lines, the scene's line table
// as the kernel reads it.  The point rule itself is ego_core.h's.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "../../include/doomgpu.h"
#include "ego_core.h"
#include "scene.hpp"

namespace dg {

// Per call: the frame size, the parameters, the scene's linedef count.
inline int ego_check_call(const Scene &sc, int W, int H, const dg_ego_map *p, std::string &err) {
    if (!p) { err = "null dg_ego_map"; return DG_ERR_INVALID; }
    if (W < 16 || H < 16 || W > 16384 || H > 16384) { err = "ego map frames need width and height in [16, 16384]"; return DG_ERR_INVALID; }
    if (!(p->scale >= 1.0f / 1024.0f && p->scale <= 64.0f)) { err = "ego map frames: scale must be finite and in [2^-10, 64]"; return DG_ERR_INVALID; }
    if (p->flags & ~(EGO_ROTATE | EGO_ARROW)) { err = "ego map frames: unknown flag bits"; return DG_ERR_INVALID; }
    if (sc.linedefs.size() > EGO_MAX_LINES) { err = "ego map frames: more than 65535 linedefs"; return DG_ERR_CAPACITY; }
    if (sc.linedefs.empty()) { err = "ego map frames: the scene has no linedefs"; return DG_ERR_INVALID; }
    return DG_OK;
}

// Per view (its trig filled).  (A comparison with a NaN is false: the negated form refuses it.)
inline int ego_check_view(const dg_view &v, std::string &err) {
    if (!(std::fabs(v.x) <= 65536.0f && std::fabs(v.y) <= 65536.0f)) { err = "ego map frames: view.x and view.y must be finite and within +-65536"; return DG_ERR_INVALID; }
    if (!(std::fabs(v.cos_a) <= 1.0f && std::fabs(v.sin_a) <= 1.0f)) { err = "ego map frames: cos_a and sin_a must be finite and within +-1"; return DG_ERR_INVALID; }
    return DG_OK;
}

inline EgoView ego_view(const dg_view &v) { return EgoView{v.x, v.y, v.cos_a, v.sin_a}; }

// draw_map_player (game.rs:287-309) in the player-centred frame: the four map-space points exactly as map_arrow_lines computes them
// (Vertex::rotate literally, the host's cosf / sinf for the two head angles) with the lengths over the scale, then the point rule.
inline int ego_arrow_lines(int W, int H, const dg_view &view, const dg_ego_map &p, dg_map_line out[3], std::string &err) {
    const float PI = 3.14159265358979323846f;                                  // std::f32::consts::PI
    const float a = view.angle, len = ((float)W / 16.0f) / p.scale, alen = ((float)W / 32.0f) / p.scale;
    const float zero = 0.0f;
    const float c = view.cos_a, s = view.sin_a;
    const float px = view.x, py = view.y;
    const float ex = px + (len * c - zero * s), ey = py + (zero * c + len * s);
    const float ar = (a - PI) - PI / 4.0f, al = (a - PI) + PI / 4.0f;
    const float cr = cosf(ar), sr = sinf(ar), cl = cosf(al), sl = sinf(al);
    const float rx = ex + (alen * cr - zero * sr), ry = ey + (zero * cr + alen * sr);
    const float lx = ex + (alen * cl - zero * sl), ly = ey + (zero * cl + alen * sl);
    const float pts[4][2] = {{px, py}, {ex, ey}, {rx, ry}, {lx, ly}};
    const EgoView v = ego_view(view);
    int32_t P[4][2];
    for (int k = 0; k < 4; k++) {
        float X, Y;
        ego_point_f(pts[k][0], pts[k][1], v, p.scale, (p.flags & EGO_ROTATE) != 0, W, H, X, Y);
        if (!(std::fabs(X) <= 16777216.0f && std::fabs(Y) <= 16777216.0f)) {      // (an angle that is not finite)
            err = "the player arrow lands beyond +-2^24 pixels of the ego map frame";
            return DG_ERR_INVALID;
        }
        P[k][0] = (int32_t)X; P[k][1] = (int32_t)Y;
    }
    out[0] = dg_map_line{P[0][0], P[0][1], P[1][0], P[1][1], EGO_YELLOW_RGB};
    out[1] = dg_map_line{P[2][0], P[2][1], P[1][0], P[1][1], EGO_YELLOW_RGB};
    out[2] = dg_map_line{P[3][0], P[3][1], P[1][0], P[1][1], EGO_YELLOW_RGB};
    return DG_OK;
}

// The scene's linedefs as dg_ego_tiles reads them: the two vertices, and ego_line_word.
inline void ego_line_table(const Scene &sc, std::vector<EgoLine> &lines, std::vector<uint32_t> &words) {
    const size_t L = sc.linedefs.size();
    lines.resize(L); words.resize(L);
    for (size_t k = 0; k < L; k++) {
        const LinedefRec &d = sc.linedefs[k];
        lines[k] = EgoLine{sc.vx[(size_t)d.v1], sc.vy[(size_t)d.v1], sc.vx[(size_t)d.v2], sc.vy[(size_t)d.v2]};
        words[k] = ego_line_word((uint32_t)k, (d.flags & 4) != 0, !(d.flags & 128));       // TWOSIDED, DONTDRAW
    }
}

// The lines of one frame in draw order (view checked, trig filled): the drawn linedefs whose bit is set in mask_row (null: all), then
// the arrow's three if the flags ask for it.
inline int ego_frame_lines(const Scene &sc, int W, int H, const dg_view &view, const dg_ego_map &p, const uint32_t *mask_row, std::vector<dg_map_line> &out,
                           std::string &err) {
    out.clear();
    const EgoView v = ego_view(view);
    const bool rotate = (p.flags & EGO_ROTATE) != 0;
    for (size_t k = 0; k < sc.linedefs.size(); k++) {
        const LinedefRec &d = sc.linedefs[k];
        if (d.flags & 128) continue;                                           // DONTDRAW
        if (mask_row && !((mask_row[k >> 5] >> (k & 31u)) & 1u)) continue;
        dg_map_line l;
        ego_point(sc.vx[(size_t)d.v1], sc.vy[(size_t)d.v1], v, p.scale, rotate, W, H, l.x0, l.y0);
        ego_point(sc.vx[(size_t)d.v2], sc.vy[(size_t)d.v2], v, p.scale, rotate, W, H, l.x1, l.y1);
        l.rgb = (d.flags & 4) ? EGO_YELLOW_RGB : EGO_RED_RGB;                  // TWOSIDED
        out.push_back(l);
    }
    if (p.flags & EGO_ARROW) {
        dg_map_line arrow[3];
        const int rc = ego_arrow_lines(W, H, view, p, arrow, err);
        if (rc) return rc;
        out.insert(out.end(), arrow, arrow + 3);
    }
    return DG_OK;
}

}  // namespace dg
