// floor_map_kernels.hpp — launch interface of the floor-textured player-centred map frames' kernels (floor_map_kernels.hip, DESIGN.md
// section 8t).
#pragma once
#include <hip/hip_runtime_api.h>

#include "ego_kernels.hpp"
#include "floor_map_core.h"

namespace dg {

// What one launch draws: frame f of E.fb = the floor under every pixel through E.views[f] (floor_map_core.h; inv = 1.0f / E.scale, from
// the host), the lines and the arrow of dg_ego_tiles on top.  cells: [n_frames][T.n_sectors]; seen: [n_frames][seen_words] sector bits,
// or null (every sector is shown).
struct FloorMapParams {
    EgoParams E;
    FloorTables T;
    const FloorCell *cells;
    const uint32_t *seen;
    uint32_t seen_words;
    float inv;
};

// dg_floor_map_tiles over every (frame, band).  The limits of launch_ego_tiles, and: cells not null, T's tables not null where their
// counts are not 0, seen null or seen_words >= ceil(T.n_sectors / 32) (else hipErrorInvalidValue).  start / stop: attached to the first /
// last dispatch.
hipError_t launch_floor_map_tiles(const FloorMapParams &p, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// dg_floor_seen_sectors: seen[f][seen_words] = the sectors of the sidedefs of every linedef whose bit is set in masks[f][mask_words], one
// lane per (frame, linedef).  The rows are cleared first, on the same stream.  n_frames x n_lines < 2^32.
hipError_t launch_floor_seen_sectors(const FloorLine *lines, uint32_t n_lines, uint32_t n_sectors, const uint32_t *masks, uint32_t mask_words, uint32_t *seen,
                                     uint32_t seen_words, int32_t n_frames, hipStream_t stream);

}  // namespace dg
