// mobj_pose_core.h — per-view map-object poses (dg_view_poses): the rows [frame][map object] FsMobj the seg walk reads
// when a batch moves objects, as one body for the host (the list walker, dg_slot_mobj_poses, tests/mobj_pose) and the device
// (mobj_pose_kernels.hip).  Two steps: every row starts as the scene's (pose_fill, one 16-byte element per lane), then every entry
// writes its object's row with the sector get_sector_from_vertex gives for the new position (pose_place, one entry per lane: a BSP
// descent with walk_core.h's test over the WalkNode table and the leaf -> sector table).  Entries are unique per (frame, object) —
// resolve_view_poses keeps the later of two — so no two lanes write one row.
// Arithmetic contract as everywhere: IEEE f32 in the reference's operand order, no contraction (the side test must not fuse).
#pragma once
#include <stdint.h>

#include "fs_core.h"
#include "walk_core.h"

namespace dg {

// One de-duplicated entry as the host ships it: object `mobj` of frame `frame` stands at (x, y) and faces `angle`.
struct PoseEntry { int32_t frame, mobj; float x, y, angle; };
static_assert(sizeof(PoseEntry) == 20, "PoseEntry layout");

struct PoseParams {
    const FsMobj *scene_rows;       // [n_mobjs] the objects as loaded
    const WalkNode *nodes;          // the BSP (walk_core.h), root = the last node
    const int32_t *leaf_sector;     // [leaves] the sector get_sector_from_vertex reports for the leaf, -1: None
    const PoseEntry *entries;       // [n_entries], unique per (frame, mobj)
    FsMobj *rows;                   // [n_frames][n_mobjs]
    int32_t root;
    uint32_t n_mobjs, n_frames, n_entries;
};

// get_sector_from_vertex (src/renderer/bsp.rs:9-44) from the root down: the sector's index, or -1 for None.  A NaN coordinate fails
// every `<=` and takes the right child each time; children precede their parents, so the descent ends whatever the floats are.
DG_HD int32_t pose_sector_at(const WalkNode *nodes, int32_t root, const int32_t *leaf_sector, float x, float y) {
    int32_t c = root;
    while (c >= 0) c = nodes[c].child[walk_left_of(nodes[c], x, y) ? 1 : 0];
    return leaf_sector[~c];
}

// Element idx of the rows (idx < n_frames * n_mobjs, row-major) becomes the scene's: one 16-byte copy (both tables start on a
// 16-byte boundary — hipMalloc's 256, the host allocator's 16 — so the device moves an element with one dwordx4 load and store).
DG_HD void pose_fill(const PoseParams &P, uint64_t idx) {
    const uint32_t mi = (uint32_t)(idx % P.n_mobjs);
    __builtin_memcpy(__builtin_assume_aligned(P.rows + idx, 16), __builtin_assume_aligned(P.scene_rows + mi, 16), sizeof(FsMobj));
}

// Entry e (e < n_entries) writes its object's row of its frame.
DG_HD void pose_place(const PoseParams &P, uint32_t e) {
    const PoseEntry en = P.entries[e];
    if (en.frame < 0 || (uint32_t)en.frame >= P.n_frames || en.mobj < 0 || (uint32_t)en.mobj >= P.n_mobjs) return;   // (the host has checked both)
    P.rows[(size_t)en.frame * P.n_mobjs + (uint32_t)en.mobj] = FsMobj{en.x, en.y, en.angle, pose_sector_at(P.nodes, P.root, P.leaf_sector, en.x, en.y)};
}

}  // namespace dg
