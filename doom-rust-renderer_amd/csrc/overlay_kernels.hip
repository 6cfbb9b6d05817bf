// overlay_kernels.hip — screen pictures over finished colour frames (dg_overlay_device, dg_slot_overlay).
//
// dg_overlay_tiles: one workgroup per tile of a rectangle record (overlay_plan.hpp: the rectangles of a frame are disjoint and hold every
// pixel its items cover), OVL_TILE_W x OVL_TILE_H pixels — a wave takes four rows of the tile one after the other, a lane one pixel of the
// row.  For its pixel a lane walks the record's items from the last to the first and stops at the first one that covers the pixel with a
// Some texel (overlay_core.h); a pixel that found one is stored, once, three bytes; any other pixel is neither read nor written.  So there
// is no read-modify-write, no atomic, and nothing depends on the order of the workgroups.
//   The record, the row and the items are the same for every lane of a wave: the record and the items are read with scalar loads (their
// index never depends on the lane), the row test and the texel row of an item are scalar arithmetic, and a wave leaves the item walk when
// all of its lanes have their colour.  Per lane: the column test, one multiply for the texel column, the two plane bytes, the palette
// word and the shade.
//   Frame offsets are 64-bit (size_t); inside a frame 3 (y W + x) < 2^30.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "overlay_kernels.hpp"

namespace dg {

namespace {

// The frames are the only memory the kernel writes.  The records and the items are read through the constant address space: nothing
// writes them while the kernel runs, and a load from there at an address that is the same in every lane is a scalar load whatever the
// compiler knows about the stores around it (through a plain pointer the item loads inside the row loop stayed vector loads).
// load_uniform(p): *p for a p that is the same in every lane.
template <class T> __device__ T load_uniform(const T *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) % 4u == 0u && alignof(T) == 4u, "whole words");
    const __attribute__((address_space(4))) uint32_t *const w = (const __attribute__((address_space(4))) uint32_t *)p;
    uint32_t words[sizeof(T) / 4u];
    for (uint32_t i = 0; i < sizeof(T) / 4u; i++) words[i] = w[i];
    T v;
    __builtin_memcpy(&v, words, sizeof(T));
    return v;
#else
    return *p;
#endif
}

__global__ __launch_bounds__(OVL_LANES) void dg_overlay_tiles(uint8_t *__restrict__ frames, const OvlRect *__restrict__ rects, const OvlItem *__restrict__ items,
                                                              const uint32_t *__restrict__ palette, const uint8_t *__restrict__ idx, const uint8_t *__restrict__ opq,
                                                              size_t frame_bytes, uint32_t W) {
    const OvlRect R = load_uniform(rects + blockIdx.y);
    if (blockIdx.x >= R.tiles) return;
    const uint32_t t = R.tile0 + blockIdx.x, trow = t / R.tiles_x, tcol = t - trow * R.tiles_x;
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t px = (int32_t)(R.x0 + tcol * OVL_TILE_W + lane);
    const int32_t y_first = (int32_t)(R.y0 + trow * OVL_TILE_H + wave * (OVL_TILE_H / 4u));
    uint8_t *const frame = frames + (size_t)R.frame * frame_bytes;
    for (int32_t py = y_first; py < y_first + (int32_t)(OVL_TILE_H / 4u) && py < (int32_t)R.y1; py++) {
        bool open = px < (int32_t)R.x1, hit = false;
        uint32_t rgb = 0;
        for (uint32_t k = R.item1; k > R.item0 && __builtin_amdgcn_ballot_w64(open) != 0ull; k--) {
            const OvlItem it = load_uniform(items + (k - 1u));
            if (py < it.y0 || py >= it.y1) continue;
            if (open && px >= it.x0 && px < it.x1) {
                const uint32_t o = ovl_texel(it, px, py);
                const uint32_t some = opq[o], v = idx[o];
                if (some) { rgb = ovl_colour(it, palette[v]); hit = true; open = false; }
            }
        }
        if (hit) {
            uint8_t *const p = frame + ((size_t)(uint32_t)py * W + (uint32_t)px) * 3u;
            p[0] = (uint8_t)rgb; p[1] = (uint8_t)(rgb >> 8); p[2] = (uint8_t)(rgb >> 16);
        }
    }
}

}  // namespace

hipError_t launch_overlay(uint8_t *frames, int W, int H, const OvlRect *rects, uint32_t n_rects, uint32_t max_tiles, const OvlItem *items, const uint32_t *palette,
                          const uint8_t *idx, const uint8_t *opq, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_rects == 0 || max_tiles == 0) return hipSuccess;
    const size_t frame_bytes = 3u * (size_t)W * (size_t)H;
    constexpr uint32_t kMaxY = 65535;                          // records per launch: the grid's y extent
    for (uint32_t r0 = 0; r0 < n_rects; r0 += kMaxY) {
        const uint32_t nr = std::min(kMaxY, n_rects - r0);
        hipEvent_t ev0 = r0 == 0 ? start : nullptr, ev1 = r0 + nr == n_rects ? stop : nullptr;
        hipExtLaunchKernelGGL(dg_overlay_tiles, dim3(max_tiles, nr), dim3(OVL_LANES), 0, stream, ev0, ev1, 0, frames, rects + r0, items, palette, idx, opq, frame_bytes, (uint32_t)W);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
