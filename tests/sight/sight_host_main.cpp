// sight_host_main.cpp — sight_core.h's traversal in the device's form, as a stand-alone program for AddressSanitizer + UBSan:
// dg_sight_queries as a host loop over "lanes", a workgroup of SIGHT_BLOCK lanes at a time, each lane with its SightLaneStack column in
// a block of exactly the kernel's LDS size (on the heap, so that a write past a column's last entry is a report).  The tables, the
// height rows, the queries and the expected results come from a file tests/test_sight_host.py writes from the WAD's lumps and
// np_sight's model:
//     u32 magic 'SGT1', n_nodes, n_leaves, n_segs, n_lines, n_sectors, row_frames, n_queries, depth
//     WalkNode[n_nodes]  FloorLeaf[n_leaves]  u32 seg_line[n_segs]  SightLine[n_lines]  FsHeights[row_frames][n_sectors]
//     dg_sight_query[n_queries]  u8 expected[n_queries]
// Usage: sight_host_main FILE...   Prints "sight_host_main: ok" when every file's results match, the BSP's depth is the file's and no
// lane's stack went past it.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/sight_core.h"

using namespace dg;

namespace {

constexpr uint32_t BLOCK = 64;                            // sight_kernels.hpp's SIGHT_BLOCK

template <class T> bool take(const std::vector<uint8_t> &file, size_t &at, size_t n, std::vector<T> &out) {
    if (n > (file.size() - at) / sizeof(T)) return false;
    out.resize(n);
    if (n) std::memcpy(out.data(), file.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return true;
}

// A lane's stack that also records how deep it went.
struct CountingStack {
    SightLaneStack s;
    uint32_t deepest = 0;
    bool push(int32_t child) {
        const bool ok = s.push(child);
        if (s.n > deepest) deepest = s.n;
        return ok;
    }
    bool pop(int32_t &child) { return s.pop(child); }
};

int run_file(const char *path) {
    std::vector<uint8_t> file;
    {
        FILE *f = std::fopen(path, "rb");
        if (!f) { std::printf("%s: cannot open\n", path); return 1; }
        uint8_t buf[65536];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
        std::fclose(f);
    }
    std::vector<uint32_t> head;
    size_t at = 0;
    if (!take(file, at, 9, head) || head[0] != 0x31544753u) { std::printf("%s: bad header\n", path); return 1; }
    const uint32_t n_nodes = head[1], n_leaves = head[2], n_segs = head[3], n_lines = head[4], n_sectors = head[5], row_frames = head[6], n_queries = head[7], depth = head[8];
    std::vector<WalkNode> nodes;
    std::vector<FloorLeaf> leaves;
    std::vector<uint32_t> seg_line;
    std::vector<SightLine> lines;
    std::vector<FsHeights> rows;
    std::vector<dg_sight_query> queries;
    std::vector<uint8_t> expected;
    if (!take(file, at, n_nodes, nodes) || !take(file, at, n_leaves, leaves) || !take(file, at, n_segs, seg_line) || !take(file, at, n_lines, lines) ||
        !take(file, at, (size_t)row_frames * n_sectors, rows) || !take(file, at, n_queries, queries) || !take(file, at, n_queries, expected) || at != file.size()) {
        std::printf("%s: truncated or oversized\n", path);
        return 1;
    }
    // exactly sized copies on the heap: an index past a table is a report
    const SightTables T{nodes.data(), n_nodes, leaves.data(), n_leaves, seg_line.data(), n_segs, lines.data(), n_lines, rows.data(), n_sectors, row_frames};
    std::vector<uint32_t> scratch(n_nodes);
    const uint32_t found = sight_depth(nodes.data(), n_nodes, scratch.data());
    if (found != depth) { std::printf("%s: depth %u, the file says %u\n", path, found, depth); return 1; }
    if (depth > SIGHT_MAX_DEPTH) { std::printf("%s: depth %u is beyond the device form's %u\n", path, depth, SIGHT_MAX_DEPTH); return 1; }
    const std::unique_ptr<int16_t[]> lds(new int16_t[SIGHT_MAX_DEPTH * BLOCK]);
    uint32_t bad = 0, deepest = 0, visible = 0;
    for (uint32_t block = 0; block * BLOCK < n_queries; block++)
        for (uint32_t lane = 0; lane < BLOCK; lane++) {
            const uint32_t i = block * BLOCK + lane;
            if (i >= n_queries) break;
            CountingStack stack{SightLaneStack{lds.get() + lane, BLOCK, 0u}};
            const uint8_t got = sight_query(T, queries[i], stack);
            if (stack.deepest > deepest) deepest = stack.deepest;
            visible += got;
            if (got != expected[i] && bad++ < 10)
                std::printf("%s: query %u (%g, %g, %g) -> (%g, %g, [%g, %g]) frame %d: %u, expected %u\n", path, i, queries[i].x0, queries[i].y0, queries[i].z0, queries[i].x1,
                            queries[i].y1, queries[i].z1_lo, queries[i].z1_hi, queries[i].frame, got, expected[i]);
        }
    if (deepest > depth) { std::printf("%s: a stack held %u entries, the BSP is %u deep\n", path, deepest, depth); return 1; }
    std::printf("%s: %u queries, %u visible, %u wrong, depth %u, deepest stack %u\n", path, n_queries, visible, bad, depth, deepest);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: sight_host_main FILE...\n"); return 2; }
    int rc = 0;
    for (int i = 1; i < argc; i++) rc |= run_file(argv[i]);
    if (!rc) std::printf("sight_host_main: ok\n");
    return rc;
}
