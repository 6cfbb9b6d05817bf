// ego_kernels.hip — player-centred map frames: the linedefs of the uploaded scene rasterised per frame, through
// that frame's view, scale and mask.  The rules are ego_core.h's and map_core.h's; everything past the point transform is integer.
//
// dg_ego_tiles   one workgroup of 256 lanes per (frame, band of whole rows, ego_band_rows).  The band's owner tile lives in LDS, one
//                uint32 per pixel, 0 = no line.  Three phases:
//                1. the scene's linedefs in chunks of EGO_CHUNK, one per lane: mask bit and drawn bit, both vertices through
//                   ego_point, the endpoints' box against the band (most lines end here, before any 64-bit division), then
//                   map_seg_make of the line translated by the band's first row.  Survivors go to a list in LDS whose capacity is the
//                   chunk's size: at a small scale a band is touched by every line of the level, so the list is not sized by the scene.
//                2. each wavefront takes the list's entries in turn, its lanes the entry's steps: atomicMax(tile[pixel], value).  The
//                   maximum over (index + 1) << 1 | yellow is the draw order whatever order the lanes ran in.  After the last chunk
//                   the arrow's three frame-clipped lines (from the host, 96 bytes per frame) with a value above every linedef's.
//                3. the tile as RGB24 into the frame, non-temporal, in the widest form that keeps every band start aligned:
//                   <.., 16> 16 pixels = three 16-byte stores per item, <.., 4> 4 pixels = three dword stores, <.., 1> bytes.
//                Every tile index and every item is bounds-checked.  <TILE, ..>: the tile's words, EGO_TILE_PX or, for frames wider
//                than that, EGO_WIDE_TILE_PX.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "ego_kernels.hpp"
#include "ego_tile_phases.h"

namespace dg {

namespace {

constexpr int kThreads = kEgoThreads;
constexpr int kMaxY = kEgoMaxY;

// The phases are ego_tile_phases.h's, shared with dg_floor_map_tiles.
template <uint32_t TILE, int PX>
__global__ void __launch_bounds__(kThreads) dg_ego_tiles(EgoParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[TILE];
    __shared__ MapSeg list[EGO_CHUNK];
    __shared__ uint32_t n_list[2];                        // chunk c appends through n_list[c & 1]; the other one is cleared meanwhile
    const uint32_t f = blockIdx.y;
    EgoBand b;
    if (!ego_band<TILE>(p.W, p.H, b)) return;
    const EgoView v = p.views[f];
    ego_tile_lines(tile, list, n_list, p.lines, p.words, p.n_lines, p.masks ? p.masks + (size_t)f * p.mask_words : nullptr,
                   p.arrow ? p.arrow + (size_t)3u * f : nullptr, v, p.scale, p.rotate != 0u, p.W, p.H, b);
    ego_tile_store<PX>(tile, ego_band_out(p.fb, f, p.W, p.H, b), b.px, [](uint32_t w) { return ego_value_rgb(w); });
}

template <uint32_t TILE>
void launch_one(int px_form, dim3 grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const EgoParams &q) {
    if (px_form == 16) hipExtLaunchKernelGGL((dg_ego_tiles<TILE, 16>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
    else if (px_form == 4) hipExtLaunchKernelGGL((dg_ego_tiles<TILE, 4>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
    else hipExtLaunchKernelGGL((dg_ego_tiles<TILE, 1>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q);
}

}  // namespace

hipError_t launch_ego_tiles(const EgoParams &p, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (p.n_frames <= 0) return hipSuccess;
    if (p.W < 1 || p.H < 1 || p.W > (int32_t)EGO_WIDE_TILE_PX || p.H > 16384 || p.n_lines > EGO_MAX_LINES || !p.views || !p.fb) return hipErrorInvalidValue;
    if (p.n_lines > 0u && (!p.lines || !p.words)) return hipErrorInvalidValue;
    if (p.masks && (size_t)p.mask_words * 32u < p.n_lines) return hipErrorInvalidValue;
    const uint32_t W = (uint32_t)p.W, H = (uint32_t)p.H, bands = ego_bands(W, H);
    const size_t fsz = (size_t)3 * W * H;
    const int px_form = (int)ego_store_px(W, H, (uint64_t)reinterpret_cast<uintptr_t>(p.fb));
    for (int f0 = 0; f0 < p.n_frames; f0 += kMaxY) {       // more frames than the grid's y extent take several launches
        const int nf = std::min(kMaxY, p.n_frames - f0);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == p.n_frames ? stop : nullptr;
        EgoParams q = p;
        q.views = p.views + f0;
        q.arrow = p.arrow ? p.arrow + (size_t)3 * f0 : nullptr;
        q.masks = p.masks ? p.masks + (size_t)f0 * p.mask_words : nullptr;
        q.fb = p.fb + (size_t)f0 * fsz;
        q.n_frames = nf;
        const dim3 grid(bands, (unsigned)nf);
        if (W > EGO_TILE_PX) launch_one<EGO_WIDE_TILE_PX>(px_form, grid, stream, ev0, ev1, q);
        else launch_one<EGO_TILE_PX>(px_form, grid, stream, ev0, ev1, q);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
