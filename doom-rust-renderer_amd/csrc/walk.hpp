// walk.hpp — host side of the player movement from recorded keys (dg_walk_*): plain host C++, no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "scene.hpp"
#include "walk_core.h"

// A play-through: the poses of all tics and the probes of their moves, worked out at creation, and the floor per tic once located
// (on the host by locate_host, or from dg_ctx_locate_walks' result by set_floors).
struct dg_walk {
    const dg::Scene *sc = nullptr;
    std::vector<dg::WalkPose> pose;         // [tics + 1]
    std::vector<float> px, py;              // the probes: the start, then every move's position in order
    std::vector<uint32_t> end_of_tic;       // [tics + 1] the last probe at or before the end of tic t
    std::vector<float> floors;              // [tics + 1] once located
    bool located = false;
    bool queued = false;                    // inside one dg_ctx_locate_walks call: already among its walks

    uint32_t tics() const { return (uint32_t)pose.size() - 1u; }
    void locate_host();
    void view_at(float timestamp, dg_view &out) const;      // located walks only
};

namespace dg {

// DG_OK and *out, or DG_ERR_INVALID with err.
int walk_create(const Scene &sc, const dg_walk_desc &d, dg_walk **out, std::string &err);

}  // namespace dg
