// explored_kernels.hpp — launch interface of the explored-map kernels (explored_kernels.hip).
//
//   seen rows   : launch_seen_lines      — label planes -> one bitset of linedefs per frame (dg_seen_lines)
//   session     : launch_seen_accumulate — the running OR of the rows along each run, and its popcounts (dg_seen_accumulate, dg_seen_counts)
//   map frames  : launch_explored_frames — the map frame of every view through that frame's line mask (dg_map_explored), then the arrow
#pragma once
#include <hip/hip_runtime_api.h>

#include "explored_core.h"
#include "map_core.h"

namespace dg {

// seen[f][words] |= the linedefs seen by frame f of id / cls (n_frames planes of W x H; id 2-byte aligned), through seg_line[n_segs].
// The rows must be zero when the kernel starts (the caller clears them on the same stream).  n_segs <= 32 * SEEN_MAX_SEG_WORDS.
hipError_t launch_seen_lines(const uint16_t *id, const uint8_t *cls, int W, int H, int n_frames, const uint32_t *seg_line, uint32_t n_segs,
                             uint32_t *seen, uint32_t words, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// The contract of dg_seen_accumulate_host on device pointers: n_frames = runs * run_len rows of `seen`; carry_in may be null (all zero);
// upto is required (n_frames rows), carry_out (runs rows), total and fresh (n_frames entries) may be null.
hipError_t launch_seen_accumulate(const uint32_t *seen, uint32_t words, int n_frames, int run_len, const uint32_t *carry_in, uint32_t *upto,
                                  uint32_t *total, uint32_t *fresh, uint32_t *carry_out, hipStream_t stream, hipEvent_t start = nullptr,
                                  hipEvent_t stop = nullptr);

// fb frame f = cover / chains picked through masks[f][words] (explored_pick), then arrow[3f .. 3f + 3) drawn on top.  words <=
// EXPLORED_MAX_WORDS.  start: on the frame kernel, stop: on the arrow kernel.
hipError_t launch_explored_frames(const uint32_t *cover, const uint32_t *chains, const uint32_t *masks, uint32_t words, const MapSeg *arrow,
                                  int n_frames, uint8_t *fb, int W, int H, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
