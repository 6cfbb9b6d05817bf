// explored_cover.hpp — host side of the explored-map frames: the linedef every drawn map line belongs to, and the cover / chain
// structure of explored_core.h built from dg_map_lines' lines (off the hot path: once per uploaded scene and frame size, one step per
// line pixel).  Used by context.cpp (the upload) and by tests/explored/explored_host_main.cpp (explored_pick against the literal rule).
#pragma once
#include <string>
#include <vector>

#include "explored_core.h"
#include "map_core.h"
#include "scene.hpp"

namespace dg {

// The LINEDEFS index of line k of map_frame_lines(view = nullptr): every linedef without DONTDRAW, in order.
inline std::vector<uint32_t> explored_line_ids(const Scene &sc) {
    std::vector<uint32_t> ids;
    for (size_t l = 0; l < sc.linedefs.size(); l++)
        if (!(sc.linedefs[l].flags & 128)) ids.push_back((uint32_t)l);
    return ids;
}

struct ExploredCover {
    std::vector<uint32_t> cover;     // W * H words
    std::vector<uint32_t> chains;    // never empty (a device copy needs an address)
};

inline int build_explored_cover(const Scene &sc, int W, int H, ExploredCover &out, std::string &err) {
    std::vector<dg_map_line> lines;
    const int rc = map_frame_lines(sc, W, H, nullptr, lines, err);
    if (rc) return rc;
    const std::vector<uint32_t> ids = explored_line_ids(sc);
    const size_t px = (size_t)W * (size_t)H;
    // every (pixel, entry) pair in draw order, then a stable counting sort by pixel: a pixel's entries stay in draw order
    std::vector<MapSeg> segs(lines.size());
    std::vector<uint32_t> count(px + 1, 0u);
    for (size_t k = 0; k < lines.size(); k++) {
        const dg_map_line &l = lines[k];
        segs[k] = map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
        for (int32_t i = 0; i < segs[k].count; i++) {
            int32_t x, y;
            map_seg_point(segs[k], (int64_t)segs[k].first + i, x, y);
            if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) count[(size_t)y * (size_t)W + (size_t)x + 1]++;
        }
    }
    for (size_t p = 0; p < px; p++) count[p + 1] += count[p];                 // count[p]: where pixel p's entries start
    if (count[px] >= (1u << 30)) { err = "explored map cover: too many line steps"; return DG_ERR_CAPACITY; }
    std::vector<uint32_t> entries(count[px]), fill(count.begin(), count.end() - 1);
    for (size_t k = 0; k < lines.size(); k++) {
        const uint32_t e = explored_entry(ids[k], lines[k].rgb == EXPLORED_YELLOW_RGB);
        for (int32_t i = 0; i < segs[k].count; i++) {
            int32_t x, y;
            map_seg_point(segs[k], (int64_t)segs[k].first + i, x, y);
            if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) entries[fill[(size_t)y * (size_t)W + (size_t)x]++] = e;
        }
    }
    out.cover.assign(px, 0u);
    out.chains.clear();
    for (size_t p = 0; p < px; p++) {
        const uint32_t lo = count[p], n = count[p + 1] - lo;
        if (n == 1) out.cover[p] = entries[lo];
        else if (n > 1) {
            out.cover[p] = EXPLORED_CHAIN | (uint32_t)out.chains.size();
            out.chains.push_back(n);
            for (uint32_t i = n; i-- > 0;) out.chains.push_back(entries[lo + i]);   // the latest line first
        }
    }
    if (out.chains.empty()) out.chains.push_back(0u);
    return DG_OK;
}

}  // namespace dg
