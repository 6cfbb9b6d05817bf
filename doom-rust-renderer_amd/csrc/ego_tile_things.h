// ego_tile_things.h — the things phase of a band workgroup, device code: the map objects' marker edges into the
// owner tile that ego_tile_lines (ego_tile_phases.h) has filled.  The tile is a maximum over values and a marker edge's value lies above
// every linedef's and below the arrow's, so the phase runs behind ego_tile_lines as it stands and the tile ends up in draw order all the
// same.  The rules are map_things_core.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "ego_tile_phases.h"
#include "map_things_kernels.hpp"

namespace dg {

// Items (object, edge), one per lane in chunks of EGO_CHUNK: the shown bit and the marker's flags, the object's place in frame f (its
// entry, else the scene's), the edge's two map points, ego_band_seg.  Survivors go into ego_tile_lines' list, then the same
// wave-per-entry atomicMax walk.  On return (behind a barrier) the tile holds the band's markers too.  Called by every lane, behind
// ego_tile_lines' last barrier.
__device__ __forceinline__ void ego_tile_things(uint32_t *tile, MapSeg *list, uint32_t *n_list, const ThingParams &T, uint32_t f, const EgoView &v, float scale,
                                                bool rotate, int32_t W, int32_t H, const EgoBand &b) {
    const uint32_t n_items = T.n_things * THING_EDGES;
    if (n_items == 0u) return;
    const uint32_t tid = threadIdx.x;
    const int32_t row0 = b.row0, rows = b.rows;
    const uint32_t *const shown = T.shown + (size_t)f * T.shown_words;
    const uint32_t e0 = T.first[f], e1 = T.first[f + 1u];
    const ThingEntry *const entries = T.entries + e0;
    const uint32_t n_entries = e1 >= e0 ? e1 - e0 : 0u;
    if (tid < 2u) n_list[tid] = 0u;                       // (ego_tile_lines left them in either state)
    __syncthreads();
    uint32_t parity = 0u;
    for (uint32_t base = 0; base < n_items; base += EGO_CHUNK, parity ^= 1u) {
        const uint32_t item = base + tid;
        if (item < n_items) {
            const uint32_t mobj = item / THING_EDGES, edge = item - mobj * THING_EDGES;
            if ((mobj >> 5) < T.shown_words) {            // (the launcher checks the row length: always)
                const MapSeg s = thing_band_seg(mobj, edge, shown, T.markers, entries, n_entries, T.places, v, scale, rotate, W, H, row0, rows);
                if (s.count > 0) {
                    const uint32_t at = atomicAdd(&n_list[parity], 1u);
                    if (at < EGO_CHUNK) list[at] = s;     // (a chunk has EGO_CHUNK items: always)
                }
            }
        }
        __syncthreads();
        const uint32_t n = min(n_list[parity], EGO_CHUNK);
        if (tid == 0u) n_list[parity ^ 1u] = 0u;          // the next chunk appends only after the barrier below
        for (uint32_t e = tid / kEgoWave; e < n; e += kEgoThreads / kEgoWave) {
            const MapSeg s = list[e];
            for (int32_t k = (int32_t)(tid % kEgoWave); k < s.count; k += kEgoWave) {
                int32_t x, y;
                map_seg_point(s, (int64_t)s.first + k, x, y);
                if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)rows) atomicMax(&tile[(uint32_t)y * (uint32_t)W + (uint32_t)x], s.rgb);
            }
        }
        __syncthreads();
    }
}

}  // namespace dg
