// tests/floor_map/floor_map_tables_main.hip — dg_floor_map_tiles on descent tables no map of the suite has (floor_map_tables.h: no nodes,
// a leaf without a sector, a leaf without segs, a chain of 200 partitions, and every index the kernel must refuse), against the rule's
// own functions on the host over tables cut to exactly their stated counts.  tests/test_floor_map_gpu.py builds it together with
// floor_map_kernels.hip and runs it.
//   The device tables carry slack past their stated counts, filled with decoys that light the pixel: an index the kernel fails to refuse
//   reads valid memory and shows as a lit pixel in a frame that is expected to be background.  The controls state the slack as part of
//   the table: the same index is then in range and the same pixels are lit.  No lines, no arrow, no mask: frames of 300x41 (two bands,
//   dword stores) and 131x67 (two bands, byte stores), three to a set, as one submission per frame size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/floor_map_kernels.hpp"
#include "floor_map_tables.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("floor_map_tables_main: line %d: %s fails\n", __LINE__, #cond); return 1; } \
    } while (0)
#define HIP(call) CHECK((call) == hipSuccess)

using namespace dg;
using namespace floor_tables_test;

template <class T> static T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size() * sizeof(T), 16)) != hipSuccess) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

static int run_set(const TableSet &s, uint64_t &lit_all) {
    CHECK(s.nodes.size() >= (size_t)s.n_nodes && s.leaves.size() >= (size_t)s.n_leaves && s.segs.size() >= (size_t)s.n_segs &&
          s.flats.size() >= (size_t)s.n_flats * 4096 && s.row.size() >= (size_t)s.n_sectors);
    Exact e;
    exact(s, e);
    WalkNode *const d_nodes = to_device(s.nodes);
    FloorLeaf *const d_leaves = to_device(s.leaves);
    FloorSeg *const d_segs = to_device(s.segs);
    uint8_t *const d_flats = to_device(s.flats);
    uint32_t *const d_palette = to_device(s.palette);
    CHECK(d_nodes && d_leaves && d_segs && d_flats && d_palette);
    const FloorTables Td{s.n_nodes ? d_nodes : nullptr, s.n_nodes, d_leaves, s.n_leaves, d_segs, s.n_segs, d_flats, s.n_flats, d_palette, s.n_sectors};
    const std::vector<TestView> views = views_of(s);
    CHECK(!views.empty() && views.size() <= 3);
    uint64_t lit = 0, px = 0;
    for (size_t first = 0; first < views.size();) {         // the views of one frame size, scale and rotation: one launch
        size_t n = 1;
        while (first + n < views.size() && views[first + n].W == views[first].W && views[first + n].H == views[first].H && views[first + n].scale == views[first].scale &&
               views[first + n].rotate == views[first].rotate)
            n++;
        const TestView &t = views[first];
        std::vector<EgoView> ev;
        for (size_t k = 0; k < n; k++) ev.push_back(views[first + k].v);
        const std::vector<FloorCell> cells = cells_of(s, (int)n);
        const size_t fsz = (size_t)3 * (size_t)t.W * (size_t)t.H;
        EgoView *const d_views = to_device(ev);
        FloorCell *const d_cells = to_device(cells);
        uint8_t *d_fb = nullptr;
        CHECK(d_views && d_cells);
        HIP(hipMalloc(&d_fb, fsz * n));
        HIP(hipMemset(d_fb, 0x5a, fsz * n));
        FloorMapParams P{};
        P.E = EgoParams{nullptr, nullptr, 0u, d_views, nullptr, nullptr, 0u, t.scale, t.rotate ? 1u : 0u, t.W, t.H, d_fb, (int32_t)n};
        P.T = Td;
        P.cells = d_cells;
        P.seen = nullptr;
        P.seen_words = 0u;
        P.inv = 1.0f / t.scale;
        HIP(launch_floor_map_tiles(P, nullptr));
        HIP(hipDeviceSynchronize());
        std::vector<uint8_t> got(fsz * n), want(fsz);
        HIP(hipMemcpy(got.data(), d_fb, got.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; k++) {
            lit += rule_frame(e.T, cells.data() + k * s.n_sectors, views[first + k], want.data());
            px += (uint64_t)t.W * (uint64_t)t.H;
            if (std::memcmp(want.data(), got.data() + fsz * k, fsz) != 0) {
                size_t bad = 0;
                for (size_t i = 0; i < fsz; i += 3) bad += std::memcmp(&want[i], &got[fsz * k + i], 3) != 0;
                std::printf("floor_map_tables_main: %s: %dx%d view %zu: %zu pixels differ from the rule's\n", s.name.c_str(), t.W, t.H, first + k, bad);
                return 1;
            }
        }
        HIP(hipFree(d_views)); HIP(hipFree(d_cells)); HIP(hipFree(d_fb));
        first += n;
    }
    if (!meets(s, lit, px)) { std::printf("floor_map_tables_main: %s: %llu of %llu pixels lit\n", s.name.c_str(), (unsigned long long)lit, (unsigned long long)px); return 1; }
    HIP(hipFree(d_nodes)); HIP(hipFree(d_leaves)); HIP(hipFree(d_segs)); HIP(hipFree(d_flats)); HIP(hipFree(d_palette));
    lit_all += lit;
    return 0;
}

int main() {
    uint64_t lit = 0;
    const std::vector<TableSet> sets = all_sets();
    CHECK(sets.size() == 15);
    for (const TableSet &s : sets)
        if (run_set(s, lit)) return 1;
    std::printf("floor_map_tables_main: ok (%zu table sets, %llu lit pixels)\n", sets.size(), (unsigned long long)lit);
    return 0;
}
