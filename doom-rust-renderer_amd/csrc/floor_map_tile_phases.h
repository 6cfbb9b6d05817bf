// floor_map_tile_phases.h — the floor phase of a band workgroup, device code, shared by dg_floor_map_tiles (floor_map_kernels.hip) and
// dg_floor_thing_tiles (map_things_kernels.hip): the per-pixel body that fills every pixel of the owner tile no line covers.  The rule
// is floor_map_core.h's; the descent's shape is described at the head of floor_map_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "ego_tile_phases.h"
#include "floor_map_kernels.hpp"

namespace dg {

// The floor phase for one pixel of a wave whose lanes all call it (want: this lane has a pixel to fill): the tile word.
__device__ __forceinline__ uint32_t floor_lane(const FloorTables &T, const FloorCell *row, const uint32_t *seen, bool want, float mx, float my) {
    int32_t c = (int32_t)T.n_nodes - 1;
    const uint64_t wm = __ballot(want);
    if (wm == 0ull) return 0u;                                                 // (the whole wave: lines only)
    const int lane0 = __ffsll((unsigned long long)wm) - 1;
    for (;;) {                                                                 // the path the wave's pixels share: c is one value, a scalar
        const int32_t cu = __builtin_amdgcn_readlane(c, lane0);
        if (cu < 0 || (uint32_t)cu >= T.n_nodes) break;                        // a leaf (or an index out of range: the walk below refuses it)
        const WalkNode n = T.nodes[cu];
        const bool left = walk_left_of(n, mx, my);
        const uint64_t lm = __ballot(want && left);
        if (lm != 0ull && lm != wm) break;                                     // they part at this node: each goes on from it alone
        c = n.child[lm ? 1 : 0];
    }
    if (want)
        while (c >= 0) {
            if ((uint32_t)c >= T.n_nodes) { c = INT32_MIN; break; }
            c = T.nodes[c].child[walk_left_of(T.nodes[c], mx, my) ? 1 : 0];
        }
    const int32_t leaf = (uint32_t)~c < T.n_leaves ? ~c : -1;
    const int32_t l0 = __builtin_amdgcn_readlane(leaf, lane0);
    int32_t sector;
    if (__ballot(want && leaf != l0) == 0ull) sector = floor_sector_of_leaf(T, l0, mx, my);       // one leaf for the wave: its segs are scalar loads
    else sector = floor_sector_of_leaf(T, leaf, mx, my);
    return want ? floor_value(T, sector, row, seen, mx, my) : 0u;
}

}  // namespace dg
