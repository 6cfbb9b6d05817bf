// walk_core.h — player movement from recorded keys (dg_walk_*): one tic of Game::process_down_keys
// (src/game.rs:314-373) and the floor lookup of update_current_player_height (:376-389, src/renderer/bsp.rs:9-44) over flat tables,
// as one body for the host path (walk.cpp) and the device path (walk_kernels.hip).
// The tic step is serial and takes the host's cosf / sinf through its Trig argument; the lookup is independent per probe.
// Arithmetic contract as everywhere: IEEE f32 in the reference's operand order, no contraction.
#pragma once
#include "../../include/doomgpu.h"
#include "rust_num.h"

namespace dg {

constexpr uint32_t WALK_MAX_TICS = 1u << 22;        // dg_walk_desc.n_tics
constexpr uint64_t WALK_MAX_PROBES = 1ull << 26;    // probes of one dg_ctx_locate_walks call
constexpr uint32_t WALK_SCAN_BLOCK = 1024;          // probes a scan workgroup covers: a power of two (walk_kernels.hpp)

// One BSP node: the partition as the NODES lump holds it and its children, [0] right, [1] left (taken when the point is left of or
// on the partition): >= 0 a node, < 0 the leaf ~child.  Children precede their parents (the loader checks it), so a descent ends.
struct WalkNode { float x, y, dx, dy; int32_t child[2]; };
// One subsector: the floor height of the sector its first seg with a sidedef on its side faces; none != 0: it has no such seg.
struct WalkLeaf { float floor; uint32_t none; };
static_assert(sizeof(WalkNode) == 24 && sizeof(WalkLeaf) == 8, "walk_core.h layouts");

struct WalkPose { float x, y, angle; };

// Vertex::is_left_of_line for a node's partition (src/map/vertexes.rs:27-34, src/renderer/bsp.rs:15-19): Scene::sector_from_vertex's test.
DG_HD bool walk_left_of(const WalkNode &n, float px, float py) {
    const float v2x = n.x + n.dx, v2y = n.y + n.dy;
    const float ax = px - n.x, ay = py - n.y;
    const float bx = v2x - n.x, by = v2y - n.y;
    return ax * by - ay * bx <= 0.0f;
}

// get_sector_from_vertex(..).floor_height from the root down; false: the point is in no sector (floor untouched).
DG_HD bool walk_floor_at(const WalkNode *nodes, int32_t root, const WalkLeaf *leaves, float x, float y, float &floor) {
    int32_t c = root;
    while (c >= 0) c = nodes[c].child[walk_left_of(nodes[c], x, y) ? 1 : 0];
    const WalkLeaf l = leaves[~c];
    if (l.none) return false;
    floor = l.floor;
    return true;
}

// The two lengths of a tic (src/game.rs:315-335).
struct WalkStep { float move_length, rotate_angle; };
DG_HD WalkStep walk_step_lengths(float turbo_f, bool shift) {
    const float duration = 1000.0f / 35.0f;
    const float rotate_factor = duration * 0.0025f;
    const float move_factor = duration * 0.291f;
    WalkStep s{move_factor * turbo_f, rotate_factor * turbo_f};
    if (shift) { s.move_length = s.move_length * 2.0f; s.rotate_angle = s.rotate_angle * 2.0f; }
    return s;
}

// One tic of process_down_keys on p.  trig(angle, c, s) gives cosf / sinf; probe(x, y) is called after each of the four moves that ran
// (the two turns leave the position where it was: their lookup repeats the previous one).
template <class Trig, class Probe> DG_HD void walk_tic(WalkPose &p, uint32_t keys, float turbo_f, Trig trig, Probe probe) {
    const bool alt = (keys & DG_KEY_ALT) != 0;
    const WalkStep st = walk_step_lengths(turbo_f, (keys & DG_KEY_SHIFT) != 0);
    const float ml = st.move_length;
    if (!alt && (keys & DG_KEY_LEFT)) p.angle += st.rotate_angle;
    if (!alt && (keys & DG_KEY_RIGHT)) p.angle -= st.rotate_angle;
    for (int k = 0; k < 4; k++) {                                  // strafe left, strafe right, forward, backward
        const uint32_t key = k == 0 ? DG_KEY_LEFT : k == 1 ? DG_KEY_RIGHT : k == 2 ? DG_KEY_UP : DG_KEY_DOWN;
        if (!(keys & key) || (k < 2 && !alt)) continue;
        float c, s;
        trig(k < 2 ? p.angle + 3.14159265358979323846f / 2.0f : p.angle, c, s);
        const float dx = ml * c - 0.0f * s, dy = 0.0f * c + ml * s;   // Vertex::new(ml, 0.0).rotate(a), src/map/vertexes.rs:20-25
        if (k & 1) { p.x = p.x - dx; p.y = p.y - dy; } else { p.x = p.x + dx; p.y = p.y + dy; }
        probe(p.x, p.y);
    }
}

// dg_walk_locate .. dg_walk_gather's arguments (walk_kernels.hip): the probes of all walks of a call, concatenated.
struct WalkParams {
    const WalkNode *nodes; const WalkLeaf *leaves;
    const float *x, *y;             // [n_probes]
    const uint8_t *first;           // [n_probes] != 0: the first probe of its walk
    const uint32_t *end_of_tic;     // [n_entries] per (walk, tic): the last probe at or before the end of that tic
    float *value;                   // [n_probes] the probe's floor (0.0 for a walk's first probe that misses)
    uint32_t *last;                 // [n_probes] valid ? index : 0, then its inclusive max-scan
    uint32_t *sums;                 // [n_blocks] per scan block its maximum, then the maximum of all blocks before it
    float *floors;                  // [n_entries]
    int32_t root;
    uint32_t n_probes, n_blocks;
    uint64_t n_entries;
};

}  // namespace dg
