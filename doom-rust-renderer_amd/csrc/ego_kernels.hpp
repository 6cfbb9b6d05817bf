// ego_kernels.hpp — launch interface of the player-centred map frames' kernel (ego_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "ego_core.h"

namespace dg {

// What one launch draws: frame f of fb = black, the linedefs of lines / words (n_lines of them, the scene's table) whose bit is set in
// masks[f][mask_words] (masks null: every line) through views[f], then arrow[3f .. 3f + 3) (frame-clipped; null: no arrow) on top.
struct EgoParams {
    const EgoLine *lines;
    const uint32_t *words;
    uint32_t n_lines;
    const EgoView *views;
    const MapSeg *arrow;
    const uint32_t *masks;
    uint32_t mask_words;
    float scale;
    uint32_t rotate;
    int32_t W, H;
    uint8_t *fb;
    int32_t n_frames;
};

// dg_ego_tiles over every (frame, band).  W, H in [1, 16384], n_lines <= EGO_MAX_LINES, masks null or mask_words >= ceil(n_lines / 32)
// (else hipErrorInvalidValue).  start / stop: attached to the first / last dispatch.
hipError_t launch_ego_tiles(const EgoParams &p, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
