// mobj_pose_core.h — per-view map-object poses (dg_view_poses): the view-row kind (view_rows_core.h) whose rows
// [frame][map object] FsMobj the seg walk reads when a batch moves objects.  Every entry writes its object's row with the sector
// get_sector_from_vertex gives for the new position: a BSP descent with walk_core.h's test over the WalkNode table and the leaf ->
// sector table.
// Arithmetic contract as everywhere: IEEE f32 in the reference's operand order, no contraction (the side test must not fuse).
#pragma once
#include <stdint.h>

#include "view_rows_core.h"
#include "walk_core.h"

namespace dg {

// get_sector_from_vertex (src/renderer/bsp.rs:9-44) from the root down: the sector's index, or -1 for None.  A NaN coordinate fails
// every `<=` and takes the right child each time; children precede their parents, so the descent ends whatever the floats are.
DG_HD int32_t pose_sector_at(const WalkNode *nodes, int32_t root, const int32_t *leaf_sector, float x, float y) {
    int32_t c = root;
    while (c >= 0) c = nodes[c].child[walk_left_of(nodes[c], x, y) ? 1 : 0];
    return leaf_sector[~c];
}

// One de-duplicated entry as the host ships it: object `mobj` of frame `frame` stands at (x, y) and faces `angle`.
struct PoseEntry { int32_t frame, mobj; float x, y, angle; };
static_assert(sizeof(PoseEntry) == 20, "PoseEntry layout");
struct PoseCtx {
    const WalkNode *nodes;          // the BSP (walk_core.h), root = the last node
    const int32_t *leaf_sector;     // [leaves] the sector get_sector_from_vertex reports for the leaf, -1: None
    int32_t root;
};
struct PoseRows {
    using Elem = FsMobj;
    using Entry = PoseEntry;
    using Ctx = PoseCtx;
    static DG_HD bool ctx_ok(const Ctx &c) { return c.nodes && c.leaf_sector && c.root >= 0; }
    static DG_HD int32_t frame(const Entry &e) { return e.frame; }
    static DG_HD int32_t item(const Entry &e) { return e.mobj; }
    static DG_HD Elem place(const Ctx &c, const Entry &e) { return FsMobj{e.x, e.y, e.angle, pose_sector_at(c.nodes, c.root, c.leaf_sector, e.x, e.y)}; }
};
using PoseParams = ViewRowParams<PoseRows>;

}  // namespace dg
