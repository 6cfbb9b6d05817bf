// tests/floor_map/floor_map_tables.h — descent tables no map of the suite has, built in memory, for tests/floor_map/floor_map_tables_main.hip
// (dg_floor_map_tiles on the GPU) and tests/floor_map/floor_map_host_main.cpp (the same functions on the host, under the sanitizers).
//
// A TableSet holds every table at its full length and, next to it, the counts it states to the rule.  Entries past a stated count are
// slack: decoys that would light the pixel if the rule read them.  The host's expected frames come from copies cut to exactly the stated
// counts (exact()): there an index the rule fails to refuse is the sanitizer's to report.  The device gets the full tables: there it reads
// valid memory and shows as a lit pixel where the expected frame is background.  No index of any set reaches past the slack: the
// largest is the stated count + 1, and every table has SLACK = 4 entries of it (flats: 2).
//
//   shapes     no nodes (the one leaf 0); a leaf without a sector next to a leaf without segs; a chain of 200 parallel partitions
//   refusals   a child >= n_nodes; a leaf >= n_leaves; a leaf's sector >= n_sectors; first > n_segs; count > n_segs - first; a cell's
//              flat >= n_flats — each on the two-room world, where the whole of room B's side then is background
//   controls   each refusal again with the stated count raised over the slack: the index is in range, the decoy is read, room B's side
//              is lit.  That is what shows that a missing check could not hide.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/floor_map_core.h"

namespace floor_tables_test {

using namespace dg;

constexpr uint32_t SLACK = 4, FLAT_SLACK = 2;
constexpr uint32_t CHAIN = 200;                               // partitions of the chain: leaves 0 .. 200, leaf i the strip i < x <= i + 1

struct TableSet {
    std::string name;
    std::vector<WalkNode> nodes;
    std::vector<FloorLeaf> leaves;
    std::vector<FloorSeg> segs;
    std::vector<uint8_t> flats;
    std::vector<uint32_t> palette;
    std::vector<FloorCell> row;                               // one frame's cells, n_sectors stated and SLACK decoys: a frame's row is row[0 .. n_sectors)
    uint32_t n_nodes, n_leaves, n_segs, n_flats, n_sectors;   // what the rule is told
    enum Expect { SOME_LIT, B_DARK, B_LIT } expect;           // of the set's frames: some pixels lit and some not; every pixel (all right of x = 256) background / lit
    bool is_chain = false;
};

// The tables cut to exactly what the set states, and the FloorTables over them.
struct Exact {
    std::vector<WalkNode> nodes;
    std::vector<FloorLeaf> leaves;
    std::vector<FloorSeg> segs;
    std::vector<uint8_t> flats;
    FloorTables T;
};
inline void exact(const TableSet &s, Exact &e) {
    e.nodes.assign(s.nodes.begin(), s.nodes.begin() + s.n_nodes);
    e.leaves.assign(s.leaves.begin(), s.leaves.begin() + s.n_leaves);
    e.segs.assign(s.segs.begin(), s.segs.begin() + s.n_segs);
    e.flats.assign(s.flats.begin(), s.flats.begin() + (size_t)s.n_flats * 4096);
    e.nodes.shrink_to_fit(); e.leaves.shrink_to_fit(); e.segs.shrink_to_fit(); e.flats.shrink_to_fit();
    e.T = FloorTables{e.nodes.empty() ? nullptr : e.nodes.data(), s.n_nodes, e.leaves.data(), s.n_leaves, e.segs.empty() ? nullptr : e.segs.data(), s.n_segs,
                      e.flats.data(), s.n_flats, s.palette.data(), s.n_sectors};
}

// The cells of n frames: every frame's row is the set's (n_sectors cells), and behind the last row the set's decoys.
inline std::vector<FloorCell> cells_of(const TableSet &s, int n) {
    std::vector<FloorCell> out;
    for (int f = 0; f < n; f++) out.insert(out.end(), s.row.begin(), s.row.begin() + s.n_sectors);
    out.insert(out.end(), s.row.begin() + s.n_sectors, s.row.end());
    return out;
}

inline void paint(TableSet &s, uint32_t n_flats_total) {
    s.flats.resize((size_t)n_flats_total * 4096);
    for (uint32_t f = 0; f < n_flats_total; f++)
        for (uint32_t y = 0; y < 64; y++)
            for (uint32_t x = 0; x < 64; x++) s.flats[(size_t)f * 4096 + y * 64 + x] = (uint8_t)((f & 1u ? 3u * x + 5u * y + f : (x ^ (y * 2u)) + 17u * f) & 255u);
    s.palette.resize(256);
    for (uint32_t i = 0; i < 256; i++) s.palette[i] = ((i * 7u + 1u) & 255u) | (((i * 13u + 50u) & 255u) << 8) | (((255u - i) | 1u) << 16);     // (no entry is black)
}

// Two square rooms of 256 units side by side (floor_map_launch_main.hip's), one node at x = 256, and a third leaf without segs that
// nothing points to: leaf 0 room A (sector 0), leaf 1 room B (sector 1), leaf 2 the whole plane (sector 0).  Then the slack.
inline TableSet two_rooms(const std::string &name) {
    TableSet s;
    s.name = name;
    s.nodes = {WalkNode{256.0f, 0.0f, 0.0f, 256.0f, {~1, ~0}}};
    const float seg[8][4] = {{0, 0, 0, 256}, {0, 256, 256, 256}, {256, 256, 256, 0}, {256, 0, 0, 0}, {256, 0, 256, 256}, {256, 256, 512, 256}, {512, 256, 512, 0}, {512, 0, 256, 0}};
    for (const auto &g : seg) s.segs.push_back(FloorSeg{g[0], g[1], g[2], g[3]});
    s.leaves = {FloorLeaf{0u, 4u, 0}, FloorLeaf{4u, 4u, 1}, FloorLeaf{0u, 0u, 0}};
    s.row = {FloorCell{0, 1.0f}, FloorCell{1, 0.75f}};
    s.n_nodes = 1; s.n_leaves = 3; s.n_segs = 8; s.n_flats = 2; s.n_sectors = 2;
    // the slack: nodes that send every point to leaf 2 (the last one a copy of the root, for the control whose root it becomes); leaves
    // without segs; segs of no length (nothing is behind them); cells of flat 0; two more flats
    for (uint32_t k = 0; k + 1 < SLACK; k++) s.nodes.push_back(WalkNode{0.0f, 0.0f, 1.0f, 0.0f, {~2, ~2}});
    s.nodes.push_back(s.nodes[0]);
    for (uint32_t k = 0; k < SLACK; k++) s.leaves.push_back(FloorLeaf{0u, 0u, 0});
    for (uint32_t k = 0; k < SLACK; k++) s.segs.push_back(FloorSeg{300.0f, 100.0f, 300.0f, 100.0f});
    for (uint32_t k = 0; k < SLACK; k++) s.row.push_back(FloorCell{0, 1.0f});
    paint(s, s.n_flats + FLAT_SLACK);
    s.expect = TableSet::SOME_LIT;
    return s;
}

// refusal k of 6, or its control (the stated count raised over the slack).
inline TableSet refusal(int k, bool control) {
    static const char *const names[6] = {"child >= n_nodes", "leaf >= n_leaves", "sector >= n_sectors", "first > n_segs", "count > n_segs - first", "flat >= n_flats"};
    TableSet s = two_rooms(std::string(control ? "control: " : "refused: ") + names[k]);
    s.expect = control ? TableSet::B_LIT : TableSet::B_DARK;
    switch (k) {
    case 0:
        s.nodes[0].child[0] = (int32_t)s.n_nodes + 1;
        s.nodes[SLACK].child[0] = (int32_t)s.n_nodes + 1;   // (the root's copy likewise)
        if (control) s.n_nodes += SLACK;                      // root = the copy; its right child is a node in range, which leads to leaf 2
        break;
    case 1:
        s.nodes[0].child[0] = ~(int32_t)(s.n_leaves + 1);
        if (control) s.n_leaves += SLACK;
        break;
    case 2:
        s.leaves[1].sector = (int32_t)s.n_sectors + 1;
        if (control) s.n_sectors += SLACK;                    // (a frame's row then is the whole of s.row)
        break;
    case 3:
        s.leaves[1] = FloorLeaf{s.n_segs + 1u, 1u, 1};
        if (control) s.n_segs += SLACK;
        break;
    case 4:
        s.leaves[1] = FloorLeaf{s.n_segs - 1u, 3u, 1};      // room B's last seg and two past the table
        if (control) s.n_segs += SLACK;
        break;
    default:
        s.row[1].flat = (int32_t)s.n_flats + 1;
        if (control) s.n_flats += FLAT_SLACK;
        break;
    }
    return s;
}

// No nodes: the one leaf 0, room A's four segs around it.
inline TableSet no_nodes() {
    TableSet s = two_rooms("no nodes");
    s.n_nodes = 0;
    return s;
}

// Left of or on x = 256 a leaf without segs (every point of it is inside: lit however far out), right of it a leaf without a sector.
inline TableSet sectorless_and_segless() {
    TableSet s = two_rooms("a leaf without a sector, a leaf without segs");
    s.nodes[0].child[1] = ~2;
    s.leaves[1].sector = -1;
    return s;
}

// CHAIN vertical partitions, node i at x = i + 1 (direction +y: left of or on it is x <= i + 1): its right child leaf i + 1, its left
// child node i - 1 (node 0: leaf 0).  The root is the last node; a point's path is up to CHAIN nodes long.  Leaf 0 (x <= 1) has one
// seg, the line x = 1 run downwards, so that a wave all in leaf 0 reads a seg; the others have none.  Four sectors in turn.
inline TableSet chain() {
    TableSet s;
    s.name = "a chain of 200 partitions";
    s.is_chain = true;
    for (uint32_t i = 0; i < CHAIN; i++) s.nodes.push_back(WalkNode{(float)(i + 1), 0.0f, 0.0f, 1.0f, {~(int32_t)(i + 1), i ? (int32_t)i - 1 : ~0}});
    s.segs = {FloorSeg{1.0f, 1.0f, 1.0f, 0.0f}};
    for (uint32_t l = 0; l <= CHAIN; l++) s.leaves.push_back(FloorLeaf{0u, l ? 0u : 1u, (int32_t)(l % 4u)});
    s.row = {FloorCell{0, 1.0f}, FloorCell{1, 0.5f}, FloorCell{2, 0.75f}, FloorCell{-1, 1.0f}};       // (every fourth strip is background)
    s.n_nodes = CHAIN; s.n_leaves = CHAIN + 1; s.n_segs = 1; s.n_flats = 3; s.n_sectors = 4;
    for (uint32_t k = 0; k < SLACK; k++) {
        s.nodes.push_back(WalkNode{0.0f, 0.0f, 1.0f, 0.0f, {~0, ~0}});
        s.leaves.push_back(FloorLeaf{0u, 0u, 0});
        s.segs.push_back(FloorSeg{0.0f, 0.0f, 0.0f, 0.0f});
        s.row.push_back(FloorCell{0, 1.0f});
    }
    paint(s, s.n_flats + FLAT_SLACK);
    s.expect = TableSet::SOME_LIT;
    return s;
}

struct TestView { int W, H; EgoView v; float scale; bool rotate; };

// The views of a set, three at the most.
inline std::vector<TestView> views_of(const TableSet &s) {
    const float c = 0.8f, sn = 0.6f;                          // (a rotation whose terms are not whole numbers)
    if (s.expect != TableSet::SOME_LIT)                       // the whole frame right of x = 256, inside room B: 300 / 2 and 131 / 2 units wide
        return {{300, 41, EgoView{420.0f, 128.0f, 1.0f, 0.0f}, 2.0f, false}, {131, 67, EgoView{384.5f, 100.25f, 1.0f, 0.0f}, 2.0f, false},
                {131, 67, EgoView{384.0f, 128.0f, c, sn}, 1.0f, true}};
    if (s.is_chain)
        return {{300, 41, EgoView{80.5f, 7.5f, 1.0f, 0.0f}, 1.0f, false},      // pixel centres on whole x: 64 lanes in 64 leaves, ties on every partition
                {131, 67, EgoView{-5000.0f, 3.0f, 1.0f, 0.0f}, 1.0f, false},   // far to the left: 200 shared levels, one leaf, its seg by scalar loads
                {131, 67, EgoView{100.0f, 0.0f, c, sn}, 0.5f, true}};
    return {{300, 41, EgoView{250.0f, 250.0f, 1.0f, 0.0f}, 1.0f, false}, {131, 67, EgoView{256.0f, 10.0f, c, sn}, 0.5f, true},
            {131, 67, EgoView{-40000.0f, 60000.0f, 1.0f, 0.0f}, 0.0009765625f, false}};     // (far out at scale 2^-10: a leaf without segs is lit there too)
}

inline std::vector<TableSet> all_sets() {
    std::vector<TableSet> out = {no_nodes(), sectorless_and_segless(), chain()};
    for (int k = 0; k < 6; k++) { out.push_back(refusal(k, false)); out.push_back(refusal(k, true)); }
    return out;
}

// One frame by the rule's own functions, no lines: 3 W H bytes.  Returns the number of lit pixels.
inline uint64_t rule_frame(const FloorTables &T, const FloorCell *row, const TestView &t, uint8_t *out) {
    const float inv = 1.0f / t.scale;
    uint64_t lit = 0;
    for (int Y = 0; Y < t.H; Y++)
        for (int X = 0; X < t.W; X++) {
            const uint32_t rgb = floor_value_rgb(floor_pixel(T, row, nullptr, X, Y, t.W, t.H, t.v, inv, t.rotate));
            uint8_t *const px = out + 3 * ((size_t)Y * (size_t)t.W + (size_t)X);
            px[0] = (uint8_t)rgb; px[1] = (uint8_t)(rgb >> 8); px[2] = (uint8_t)(rgb >> 16);
            lit += rgb != 0u;
        }
    return lit;
}

// Do the lit pixels of the set's frames together, of px pixels, meet what the set expects?
inline bool meets(const TableSet &s, uint64_t lit, uint64_t px) {
    return s.expect == TableSet::B_DARK ? lit == 0 : s.expect == TableSet::B_LIT ? lit == px : lit > 0 && lit < px;
}

}  // namespace floor_tables_test
