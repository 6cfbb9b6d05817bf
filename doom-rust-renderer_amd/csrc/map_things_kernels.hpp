// map_things_kernels.hpp — launch interface of the map frames with map-object markers (map_things_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "floor_map_kernels.hpp"
#include "map_things_core.h"

namespace dg {

// What the things phase of a launch reads besides the frame's view: the scene's marker and place tables (n_things of each), and per
// frame f its shown bits shown[f][shown_words] and its pose entries entries[first[f] .. first[f + 1]) sorted by object (first:
// n_frames + 1 words).  n_things == 0: no markers, nothing else is read.
struct ThingParams {
    const ThingMarker *markers;
    const ThingPlace *places;
    uint32_t n_things;
    const uint32_t *shown;
    uint32_t shown_words;
    const ThingEntry *entries;
    const uint32_t *first;
};

// dg_ego_thing_tiles over every (frame, band): launch_ego_tiles' frame with the markers between the linedefs and the arrow.  Its limits,
// and: n_things <= THING_MAX; with n_things > 0 no table null and shown_words >= ceil(n_things / 32) (else hipErrorInvalidValue).
hipError_t launch_ego_thing_tiles(const EgoParams &p, const ThingParams &t, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// dg_floor_thing_tiles: launch_floor_map_tiles' frame likewise.
hipError_t launch_floor_thing_tiles(const FloorMapParams &p, const ThingParams &t, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
