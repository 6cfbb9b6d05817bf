// walk.cpp — host side of the player movement from recorded keys (dg_walk_*): the serial pose integration with the
// host's cosf / sinf, the probe list, and the host path of the floor lookup (walk_core.h's bodies, one probe after the other).
#include "walk.hpp"

#include <cmath>
#include <memory>

#include "frontend.hpp"

using namespace dg;

namespace dg {

int walk_create(const Scene &sc, const dg_walk_desc &d, dg_walk **out, std::string &err) {
    if (d.n_tics > WALK_MAX_TICS) { err = "n_tics above 1 << 22"; return DG_ERR_INVALID; }
    if (d.n_tics > 0 && !d.keys) { err = "keys is NULL"; return DG_ERR_INVALID; }
    if (d.turbo < -32768 || d.turbo > 32767) { err = "turbo outside i16"; return DG_ERR_INVALID; }
    if (d.from_player_start && !sc.has_start) { err = "Could not find thing of type 1 (src/map/things.rs:46-55)"; return DG_ERR_INVALID; }
    std::unique_ptr<dg_walk> w(new dg_walk);
    w->sc = &sc;
    WalkPose p = d.from_player_start ? WalkPose{sc.start_x, sc.start_y, sc.start_angle} : WalkPose{d.x, d.y, d.angle};
    const float turbo_f = (float)d.turbo / 100.0f;                          // src/game.rs:178
    w->pose.reserve((size_t)d.n_tics + 1);
    w->end_of_tic.reserve((size_t)d.n_tics + 1);
    auto probe = [&](float x, float y) { w->px.push_back(x); w->py.push_back(y); };
    auto trig = [](float a, float &c, float &s) { c = cosf(a); s = sinf(a); };
    probe(p.x, p.y);
    w->pose.push_back(p);
    w->end_of_tic.push_back(0u);
    for (uint32_t t = 0; t < d.n_tics; t++) {
        walk_tic(p, d.keys[t], turbo_f, trig, probe);
        w->pose.push_back(p);
        w->end_of_tic.push_back((uint32_t)w->px.size() - 1u);
    }
    *out = w.release();
    return DG_OK;
}

}  // namespace dg

void dg_walk::locate_host() {
    if (located) return;
    const int32_t root = (int32_t)sc->walk_nodes.size() - 1;
    floors.resize(pose.size());
    float cur = 0.0f;
    size_t i = 0;
    for (size_t t = 0; t < pose.size(); t++) {
        for (; i <= end_of_tic[t]; i++) (void)walk_floor_at(sc->walk_nodes.data(), root, sc->walk_leaves.data(), px[i], py[i], cur);
        floors[t] = cur;
    }
    located = true;
}

void dg_walk::view_at(float timestamp, dg_view &out) const {
    const uint32_t T = fs_tics(timestamp), t = T < tics() ? T : tics();
    const WalkPose &p = pose[t];
    out = dg_view{p.x, p.y, p.angle, floors[t], 0.0f, 0.0f, 0.0f, 0.0f, timestamp, 0};
    fill_view_trig(out);
}
