// floor_map_kernels.hip — floor-textured player-centred map frames: dg_ego_tiles' lines over the sectors' floor
// textures.  The rule is floor_map_core.h's; the band decomposition, the owner tile and phases 1, 2 and the resolve are
// ego_tile_phases.h's, shared with dg_ego_tiles.
//
// dg_floor_map_tiles     one workgroup of 256 lanes per (frame, band).  Behind phases 1 and 2 the floor phase: the band's pixels in
//                        runs of 256, one per lane, neighbours in a row.  A pixel whose tile word is still 0 takes the rule's steps:
//                        its map point; the BSP descent; the leaf's segs; the sector's cell of the frame; the texel; the shade.  Its
//                        word becomes FLOOR_VALUE | RGB24 (or stays 0: background), and the resolve phase stores every pixel once
//                        in dg_ego_tiles' three forms, through floor_value_rgb.  Nothing reads the frame.
//                        The descent is per pixel, by walk_left_of on the pixel's own point: no block shortcut.  What makes it
//                        affordable is that the 64 pixels of a wave are neighbours in a row and share most of their path: while
//                        every lane takes the same child the node index is one value (readlane of the first lane with a pixel: a
//                        scalar register, so the node's 24 bytes are one scalar load and the agreement one ballot); at the first
//                        node where the lanes part each goes on alone from that node.  A wave that ends in one leaf reads its segs
//                        by scalar loads too.  Every index read from a table is checked.  (Measured next to a plain per-lane
//                        descent and to lanes taking turns at the first lane's node: DESIGN.md section 8t.)
// dg_floor_seen_sectors  one lane per (frame, linedef): a linedef whose bit is set in the frame's mask row sets the bits of its two
//                        sidedefs' sectors in the frame's sector row (atomicOr).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "ego_tile_phases.h"
#include "floor_map_kernels.hpp"
#include "floor_map_tile_phases.h"

namespace dg {

namespace {

constexpr int kThreads = kEgoThreads;
constexpr int kMaxY = kEgoMaxY;

// The per-pixel body, floor_lane, is floor_map_tile_phases.h's, shared with dg_floor_thing_tiles.
template <uint32_t TILE, int PX>
__global__ void __launch_bounds__(kThreads) dg_floor_map_tiles(FloorMapParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[TILE];
    __shared__ MapSeg list[EGO_CHUNK];
    __shared__ uint32_t n_list[2];
    const EgoParams &E = p.E;
    const uint32_t tid = threadIdx.x, f = blockIdx.y;
    const int32_t W = E.W, H = E.H;
    EgoBand b;
    if (!ego_band<TILE>(W, H, b)) return;
    const EgoView v = E.views[f];
    const bool rotate = E.rotate != 0u;
    ego_tile_lines(tile, list, n_list, E.lines, E.words, E.n_lines, E.masks ? E.masks + (size_t)f * E.mask_words : nullptr,
                   E.arrow ? E.arrow + (size_t)3u * f : nullptr, v, E.scale, rotate, W, H, b);
    const FloorCell *const row = p.cells + (size_t)f * p.T.n_sectors;
    const uint32_t *const seen = p.seen ? p.seen + (size_t)f * p.seen_words : nullptr;
    for (uint32_t j0 = 0; j0 < b.px; j0 += kThreads) {    // (the same trips for every lane: floor_lane's waves stay whole)
        const uint32_t j = j0 + tid;
        const bool want = j < b.px && tile[j] == 0u;
        float mx = 0.0f, my = 0.0f;
        if (want) {
            const uint32_t y = j / (uint32_t)W, x = j - y * (uint32_t)W;       // (an index, not the rule's arithmetic)
            floor_map_point((int32_t)x, b.row0 + (int32_t)y, W, H, v, p.inv, rotate, mx, my);
        }
        const uint32_t value = floor_lane(p.T, row, seen, want, mx, my);
        if (want) tile[j] = value;                        // j < px <= TILE
    }
    __syncthreads();
    ego_tile_store<PX>(tile, ego_band_out(E.fb, f, W, H, b), b.px, [](uint32_t w) { return floor_value_rgb(w); });
}

__global__ void __launch_bounds__(kThreads) dg_floor_seen_sectors(const FloorLine *__restrict__ lines, uint32_t n_lines, uint32_t n_sectors,
                                                                  const uint32_t *__restrict__ masks, uint32_t mask_words, uint32_t *__restrict__ seen,
                                                                  uint32_t seen_words) {
    const uint32_t l = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
    if (l >= n_lines || (l >> 5) >= mask_words) return;
    if (!floor_seen_line(masks + (size_t)f * mask_words, l)) return;
    const FloorLine ln = lines[l];
    uint32_t *const row = seen + (size_t)f * seen_words;
    for (const int32_t s : {ln.front, ln.back})
        if (s >= 0 && (uint32_t)s < n_sectors && ((uint32_t)s >> 5) < seen_words) atomicOr(&row[(uint32_t)s >> 5], 1u << ((uint32_t)s & 31u));
}

template <uint32_t TILE>
void launch_one(int px_form, dim3 grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const FloorMapParams &q) {
    if (px_form == 16) hipExtLaunchKernelGGL((dg_floor_map_tiles<TILE, 16>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
    else if (px_form == 4) hipExtLaunchKernelGGL((dg_floor_map_tiles<TILE, 4>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
    else hipExtLaunchKernelGGL((dg_floor_map_tiles<TILE, 1>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
}

}  // namespace

hipError_t launch_floor_map_tiles(const FloorMapParams &p, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    const EgoParams &E = p.E;
    const FloorTables &T = p.T;
    if (E.n_frames <= 0) return hipSuccess;
    if (E.W < 1 || E.H < 1 || E.W > (int32_t)EGO_WIDE_TILE_PX || E.H > 16384 || E.n_lines > EGO_MAX_LINES || !E.views || !E.fb) return hipErrorInvalidValue;
    if (E.n_lines > 0u && (!E.lines || !E.words)) return hipErrorInvalidValue;
    if (E.masks && (size_t)E.mask_words * 32u < E.n_lines) return hipErrorInvalidValue;
    if (!p.cells || !T.palette || !T.leaves || T.n_leaves == 0u || T.n_sectors == 0u || (T.n_nodes && !T.nodes) || (T.n_segs && !T.segs) || (T.n_flats && !T.flats))
        return hipErrorInvalidValue;
    if (T.n_nodes > 0x7fffffffu || (p.seen && (size_t)p.seen_words * 32u < T.n_sectors)) return hipErrorInvalidValue;
    const uint32_t W = (uint32_t)E.W, H = (uint32_t)E.H, bands = ego_bands(W, H);
    const size_t fsz = (size_t)3 * W * H;
    const int px_form = (int)ego_store_px(W, H, (uint64_t)reinterpret_cast<uintptr_t>(E.fb));
    for (int f0 = 0; f0 < E.n_frames; f0 += kMaxY) {       // more frames than the grid's y extent take several launches
        const int nf = std::min(kMaxY, E.n_frames - f0);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == E.n_frames ? stop : nullptr;
        FloorMapParams q = p;
        q.E.views = E.views + f0;
        q.E.arrow = E.arrow ? E.arrow + (size_t)3 * f0 : nullptr;
        q.E.masks = E.masks ? E.masks + (size_t)f0 * E.mask_words : nullptr;
        q.E.fb = E.fb + (size_t)f0 * fsz;
        q.E.n_frames = nf;
        q.cells = p.cells + (size_t)f0 * T.n_sectors;
        q.seen = p.seen ? p.seen + (size_t)f0 * p.seen_words : nullptr;
        const dim3 grid(bands, (unsigned)nf);
        if (W > EGO_TILE_PX) launch_one<EGO_WIDE_TILE_PX>(px_form, grid, stream, ev0, ev1, q);
        else launch_one<EGO_TILE_PX>(px_form, grid, stream, ev0, ev1, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_floor_seen_sectors(const FloorLine *lines, uint32_t n_lines, uint32_t n_sectors, const uint32_t *masks, uint32_t mask_words, uint32_t *seen,
                                     uint32_t seen_words, int32_t n_frames, hipStream_t stream) {
    if (n_frames <= 0) return hipSuccess;
    if (!lines || !masks || !seen || n_lines == 0u || (size_t)mask_words * 32u < n_lines || (size_t)seen_words * 32u < n_sectors) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(seen, 0, (size_t)n_frames * seen_words * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxY) {
        const int nf = std::min(kMaxY, n_frames - f0);
        hipLaunchKernelGGL(dg_floor_seen_sectors, dim3((n_lines + kThreads - 1) / kThreads, (unsigned)nf), dim3(kThreads), 0, stream, lines, n_lines, n_sectors,
                           masks + (size_t)f0 * mask_words, mask_words, seen + (size_t)f0 * seen_words, seen_words);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
