// sight_core.h — the rule of the line-of-sight queries (dg_sight_*) as host/device inline functions: which leaves
// of the BSP a sight line visits, what every linedef it crosses there does to it, and the query a (view, map object) pair stands for.
// sight_kernels.hip runs them on the GPU, sight_host.hpp on the host (dg_sight_host, dg_sight_mobjs_host), and
// tests/sight/sight_host_main.cpp runs the traversal in the device's form as a host loop over "lanes".
//
// A query (frame, x0, y0, z0, x1, y1, z1_lo, z1_hi): the line from S = (x0, y0) at height z0 to E = (x1, y1), whose target spans
// [z1_lo, z1_hi]; sector heights from row `frame`.  Every operation in f32 in the order written, no contraction (the units are built
// with -ffp-contract=off), `/` the correctly rounded division.  sgn(c) is -1, 0 or +1; cross(P; A, D) = (P.x - A.x) * D.y - (P.y - A.y) * D.x.
//     out of contract   one of the seven floats not finite or beyond 65536 in magnitude: 0
//     start             lo = z1_lo - z0, hi = z1_hi - z0
//     leaves            from the root (n_nodes - 1; no nodes: the one leaf 0); at a node with b = ((n.x + n.dx) - n.x, (n.y + n.dy) - n.y)
//                       (walk_left_of's operands): cS = cross(S; n, b), cE = cross(E; n, b); the near child is child[1] if cS <= 0 else
//                       child[0] and is always visited; the far child too, unless cE < 0 with near child[1] or cE > 0 with near child[0]
//     per leaf          every seg in lump order, its linedef L with vertices A -> B:
//                       d = E - S, t1 = cross(A; S, d), t2 = cross(B; S, d): sgn(t1) == sgn(t2) skips L
//                       l = B - A, u1 = cross(S; A, l), u2 = cross(E; A, l): sgn(u1) == sgn(u2) skips L
//                       L without the two-sided flag or without one of its sidedefs: blocked
//                       fh, fc, bh, bc the front and back sectors' heights of the row as f32: fh == bh and fc == bc skips L
//                       top = min(fc, bc), bot = max(fh, bh): bot >= top: blocked
//                       frac = u1 / (u1 - u2); if frac > 0:  fh != bh: lo = max(lo, (bot - z0) / frac);  fc != bc: hi = min(hi, (top - z0) / frac)
//     result            1 iff nothing blocked and hi > lo at the end
// Every step is a max into lo, a min into hi or an OR into blocked, so a linedef met twice (through two of its segs) changes nothing,
// and neither the visiting order nor an early exit changes the result: sight_traverse stops at the first block and as soon as
// hi <= lo (lo only rises, hi only falls).
//
// The pending far children are kept on a stack the caller provides (push / pop), one entry per node of the path at the most: a scene
// whose BSP is `depth` nodes deep (sight_depth) never holds more than `depth` entries.  The device's stack is SightLaneStack, a column of
// SIGHT_MAX_DEPTH 16-bit entries per lane in LDS; the host twin's grows as it has to.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "floor_map_core.h"
#include "fs_core.h"
#include "walk_core.h"

namespace dg {

constexpr uint32_t SIGHT_MAX_DEPTH = 64;                  // entries of a lane's stack: the deepest BSP the device calls take
constexpr uint32_t SIGHT_MAX_QUERIES = 1u << 20;          // dg_sight_host / dg_sight_device: queries of one call
constexpr uint32_t SIGHT_TWO_SIDED = 0x0004u;             // the linedef flag
constexpr float SIGHT_MAX_COORD = 65536.0f;

// One linedef as a sight line meets it: its vertices, the sectors its two sidedefs face (-1: no sidedef) and its flags.
struct SightLine { float ax, ay, bx, by; int32_t front, back; uint32_t flags, pad; };
static_assert(sizeof(SightLine) == 32, "SightLine");
// A viewer of the mobjs form: the view's (x, y) and z0 = view.floor_height + eye_height.
struct SightView { float x, y, z0, pad; };
static_assert(sizeof(SightView) == 16, "SightView");

// The scene's tables as the traversal reads them (device or host memory), and the height rows [row_frames][n_sectors]; row_frames 1:
// every frame reads the one row.
struct SightTables {
    const WalkNode *nodes; uint32_t n_nodes;
    const FloorLeaf *leaves; uint32_t n_leaves;           // first / count: the leaf's segs (the sector is not read)
    const uint32_t *seg_line; uint32_t n_segs;            // seg -> linedef
    const SightLine *lines; uint32_t n_lines;
    const FsHeights *rows; uint32_t n_sectors, row_frames;
};
DG_HD const FsHeights *sight_row(const SightTables &t, int32_t frame) { return t.rows + (t.row_frames > 1 ? (size_t)frame * t.n_sectors : (size_t)0); }

DG_HD int32_t sight_sgn(float c) { return c < 0.0f ? -1 : (c > 0.0f ? 1 : 0); }
DG_HD float sight_cross(float px, float py, float ax, float ay, float dx, float dy) { return (px - ax) * dy - (py - ay) * dx; }
DG_HD bool sight_coord_ok(float v) { return v >= -SIGHT_MAX_COORD && v <= SIGHT_MAX_COORD; }      // (false for a NaN and for an infinity)
DG_HD bool sight_in_contract(const dg_sight_query &q) {
    return sight_coord_ok(q.x0) && sight_coord_ok(q.y0) && sight_coord_ok(q.z0) && sight_coord_ok(q.x1) && sight_coord_ok(q.y1) && sight_coord_ok(q.z1_lo) &&
           sight_coord_ok(q.z1_hi);
}

// What a query carries through its traversal.
struct SightState { float lo, hi; bool blocked; };
DG_HD bool sight_open(const SightState &s) { return !s.blocked && s.hi > s.lo; }

// One linedef of a visited leaf.
DG_HD void sight_line_step(const SightLine &L, const FsHeights *row, uint32_t n_sectors, const dg_sight_query &q, SightState &s) {
    const float dx = q.x1 - q.x0, dy = q.y1 - q.y0;
    const float t1 = sight_cross(L.ax, L.ay, q.x0, q.y0, dx, dy), t2 = sight_cross(L.bx, L.by, q.x0, q.y0, dx, dy);
    if (sight_sgn(t1) == sight_sgn(t2)) return;
    const float lx = L.bx - L.ax, ly = L.by - L.ay;
    const float u1 = sight_cross(q.x0, q.y0, L.ax, L.ay, lx, ly), u2 = sight_cross(q.x1, q.y1, L.ax, L.ay, lx, ly);
    if (sight_sgn(u1) == sight_sgn(u2)) return;
    if (!(L.flags & SIGHT_TWO_SIDED) || L.front < 0 || L.back < 0 || (uint32_t)L.front >= n_sectors || (uint32_t)L.back >= n_sectors) { s.blocked = true; return; }
    const FsHeights f = row[L.front], b = row[L.back];
    const float fh = (float)f.floor_h, fc = (float)f.ceil_h, bh = (float)b.floor_h, bc = (float)b.ceil_h;
    if (fh == bh && fc == bc) return;
    const float top = fc < bc ? fc : bc, bot = fh > bh ? fh : bh;
    if (bot >= top) { s.blocked = true; return; }
    const float frac = u1 / (u1 - u2);
    if (frac > 0.0f) {
        if (fh != bh) { const float v = (bot - q.z0) / frac; s.lo = s.lo > v ? s.lo : v; }
        if (fc != bc) { const float v = (top - q.z0) / frac; s.hi = s.hi < v ? s.hi : v; }
    }
}

// Every seg of one leaf, in lump order, until the query closes.  A leaf or a seg the tables do not hold is passed over (never, for
// tables built by sight_tables).
DG_HD void sight_leaf_step(const SightTables &t, const FsHeights *row, uint32_t leaf, const dg_sight_query &q, SightState &s) {
    if (leaf >= t.n_leaves) return;
    const FloorLeaf l = t.leaves[leaf];
    if (l.first > t.n_segs || l.count > t.n_segs - l.first) return;
    for (uint32_t k = 0; k < l.count && sight_open(s); k++) {
        const uint32_t line = t.seg_line[l.first + k];
        if (line < t.n_lines) sight_line_step(t.lines[line], row, t.n_sectors, q, s);
    }
}

// At a node: the child on S's side, and whether the other one is visited too.
DG_HD void sight_node_step(const WalkNode &n, const dg_sight_query &q, int32_t &near, int32_t &far, bool &both) {
    const float bx = (n.x + n.dx) - n.x, by = (n.y + n.dy) - n.y;
    const float cS = sight_cross(q.x0, q.y0, n.x, n.y, bx, by), cE = sight_cross(q.x1, q.y1, n.x, n.y, bx, by);
    const bool left = cS <= 0.0f;
    near = n.child[left ? 1 : 0];
    far = n.child[left ? 0 : 1];
    both = !(left ? cE < 0.0f : cE > 0.0f);
}

// The traversal of one query (in contract, frame in range): 1 visible, 0 not.  Stack: bool push(int32_t child) — false when it is
// full, which ends the query as not visible (never, on a scene the host let through: sight_depth <= the stack's capacity) — and
// bool pop(int32_t &child), false when it is empty.
template <class Stack> DG_HD uint8_t sight_traverse(const SightTables &t, const FsHeights *row, const dg_sight_query &q, Stack &stack) {
    SightState s{q.z1_lo - q.z0, q.z1_hi - q.z0, false};
    int32_t c = t.n_nodes ? (int32_t)t.n_nodes - 1 : ~0;
    while (sight_open(s)) {
        while (c >= 0) {
            if ((uint32_t)c >= t.n_nodes) return 0;       // (never: the loader checks every child)
            int32_t near, far;
            bool both;
            sight_node_step(t.nodes[c], q, near, far, both);
            if (both && !stack.push(far)) return 0;
            c = near;
        }
        sight_leaf_step(t, row, (uint32_t)~c, q, s);
        if (!stack.pop(c)) break;
    }
    return sight_open(s) ? 1 : 0;
}
// ... of a query as a caller hands it over, over its frame's row (`row`: that row when the caller has it at hand — dg_sight_mobjs, whose
// wavefronts share a frame).  The stack must be empty.
template <class Stack> DG_HD uint8_t sight_query(const SightTables &t, const dg_sight_query &q, Stack &stack, const FsHeights *row = nullptr) {
    if (!sight_in_contract(q) || q.frame < 0 || (t.row_frames > 1 && (uint32_t)q.frame >= t.row_frames)) return 0;
    return sight_traverse(t, row ? row : sight_row(t, q.frame), q, stack);
}

// The device's stack: entry k of a lane at base[k * stride], SIGHT_MAX_DEPTH entries, each a child as the node table holds it (a node
// index below 32768, or ~leaf down to -32768: the host checks that both fit).
struct SightLaneStack {
    int16_t *base;
    uint32_t stride, n;
    DG_HD bool push(int32_t child) {
        if (n >= SIGHT_MAX_DEPTH) return false;
        base[(size_t)n * stride] = (int16_t)child;
        n++;
        return true;
    }
    DG_HD bool pop(int32_t &child) {
        if (n == 0) return false;
        n--;
        child = base[(size_t)n * stride];
        return true;
    }
};

// The query of (viewer, map object `pose`) in frame `frame`, false when the object is left out: its sector is none, or its height is
// not positive (the caller's way to leave an object out; a NaN height too).
DG_HD bool sight_mobj_query(const SightTables &t, int32_t frame, const SightView &v, const FsMobj &pose, float height, dg_sight_query &q) {
    if (pose.sector < 0 || (uint32_t)pose.sector >= t.n_sectors || !(height > 0.0f)) return false;
    const float z1_lo = (float)sight_row(t, frame)[pose.sector].floor_h;
    q = dg_sight_query{frame, v.x, v.y, v.z0, pose.x, pose.y, z1_lo, z1_lo + height};
    return true;
}

// The nodes on the longest way from the root to a leaf, from `depth` [n_nodes] scratch; children precede their parents.
inline uint32_t sight_depth(const WalkNode *nodes, uint32_t n_nodes, uint32_t *depth) {
    uint32_t deepest = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
        uint32_t d = 0;
        for (const int32_t c : nodes[i].child)
            if (c >= 0 && (uint32_t)c < i && depth[c] > d) d = depth[c];
        depth[i] = d + 1;
        deepest = depth[i];                               // (the root is the last node)
    }
    return deepest;
}

}  // namespace dg
