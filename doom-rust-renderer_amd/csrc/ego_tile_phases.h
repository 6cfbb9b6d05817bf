// ego_tile_phases.h — the phases of a band workgroup that dg_ego_tiles (ego_kernels.hip) and dg_floor_map_tiles (floor_map_kernels.hip)
// share, device code: the band of a workgroup, the owner tile cleared, phases 1 and 2 (the linedefs and the arrow into the tile by
// atomicMax) and the resolve phase's three store forms over a colour function of the tile word.  The rules are ego_core.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "ego_kernels.hpp"

namespace dg {

typedef uint32_t ego_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kEgoThreads = 256;
constexpr int kEgoWave = 64;
constexpr int kEgoMaxY = 65535;                           // frames per launch: the grid's y extent

struct EgoBand { int32_t row0, rows; uint32_t px; };      // the workgroup's rows of the frame and their pixels

// The band of workgroup blockIdx.x in a frame W x H whose tile has TILE words; false: nothing to do (never, for the launchers' grids).
template <uint32_t TILE> __device__ __forceinline__ bool ego_band(int32_t W, int32_t H, EgoBand &b) {
    const uint32_t band_rows = ego_band_rows((uint32_t)W);
    b.row0 = (int32_t)(blockIdx.x * band_rows);
    if (b.row0 >= H) return false;                        // (the grid has ego_bands bands: never)
    b.rows = min((int32_t)band_rows, H - b.row0);
    b.px = (uint32_t)b.rows * (uint32_t)W;
    return b.px <= TILE;                                  // (the launcher picks TILE so: always)
}

// The tile cleared, then phases 1 and 2 of frame f: on return (behind a barrier) the tile holds the band's lines and the arrow.
// lines / words / n_lines: the scene's table; mask: the frame's row or null; arrow: the frame's three lines or null.
__device__ __forceinline__ void ego_tile_lines(uint32_t *tile, MapSeg *list, uint32_t *n_list, const EgoLine *lines, const uint32_t *words, uint32_t n_lines,
                                               const uint32_t *mask, const MapSeg *arrow, const EgoView &v, float scale, bool rotate, int32_t W, int32_t H,
                                               const EgoBand &b) {
    const uint32_t tid = threadIdx.x;
    const int32_t row0 = b.row0, rows = b.rows;
    for (uint32_t i = 4u * tid; i < b.px; i += 4u * kEgoThreads)     // i + 3 < TILE: both are multiples of 4
        *reinterpret_cast<uint4 *>(&tile[i]) = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 2u) n_list[tid] = 0u;
    __syncthreads();
    uint32_t parity = 0u;
    for (uint32_t base = 0; base < n_lines; base += EGO_CHUNK, parity ^= 1u) {
        const uint32_t l = base + tid;
        if (l < n_lines) {
            const uint32_t w = words[l];
            if ((w & EGO_DRAWN) && (!mask || ((mask[l >> 5] >> (l & 31u)) & 1u))) {
                const MapSeg s = ego_band_seg(lines[l], w & ~EGO_DRAWN, v, scale, rotate, W, H, row0, rows);
                if (s.count > 0) {
                    const uint32_t at = atomicAdd(&n_list[parity], 1u);
                    if (at < EGO_CHUNK) list[at] = s;     // (a chunk has EGO_CHUNK lines: always)
                }
            }
        }
        __syncthreads();
        const uint32_t n = min(n_list[parity], EGO_CHUNK);
        if (tid == 0u) n_list[parity ^ 1u] = 0u;          // the next chunk appends only after the barrier below
        for (uint32_t e = tid / kEgoWave; e < n; e += kEgoThreads / kEgoWave) {
            const MapSeg s = list[e];
            for (int32_t k = (int32_t)(tid % kEgoWave); k < s.count; k += kEgoWave) {
                int32_t x, y;
                map_seg_point(s, (int64_t)s.first + k, x, y);
                if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)rows) atomicMax(&tile[(uint32_t)y * (uint32_t)W + (uint32_t)x], s.rgb);
            }
        }
        __syncthreads();
    }
    if (arrow) {
        for (uint32_t a = 0; a < 3u; a++) {
            const MapSeg s = arrow[a];
            int32_t lo, hi;
            ego_seg_rows(s, lo, hi);
            if (s.count <= 0 || hi < row0 || lo >= row0 + rows) continue;
            for (int32_t k = (int32_t)tid; k < s.count; k += kEgoThreads) {
                int32_t x, y;
                map_seg_point(s, (int64_t)s.first + k, x, y);
                y -= row0;
                if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)rows) atomicMax(&tile[(uint32_t)y * (uint32_t)W + (uint32_t)x], EGO_ARROW_VALUE);
            }
        }
        __syncthreads();
    }
}

// The resolve phase: the band's px tile words as RGB24 at out, every pixel stored once, non-temporal, PX pixels per item (PX divides px:
// ego_store_px).  rgb(word): the colour of a tile word.
template <int PX, class Rgb> __device__ __forceinline__ void ego_tile_store(const uint32_t *tile, uint8_t *out, uint32_t px, Rgb rgb) {
    const uint32_t tid = threadIdx.x;
    const uint32_t n_items = px / PX;
    for (uint32_t j = tid; j < n_items; j += kEgoThreads) {
        if constexpr (PX == 1) {
            const uint32_t c = rgb(tile[j]);
            uint8_t *const o = out + 3u * (size_t)j;
            o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
        } else if constexpr (PX == 4) {
            const uint4 t = *reinterpret_cast<const uint4 *>(&tile[4u * j]);
            uint32_t o0, o1, o2;
            ego_pack4_rgb(rgb(t.x), rgb(t.y), rgb(t.z), rgb(t.w), o0, o1, o2);
            uint32_t *const dst = reinterpret_cast<uint32_t *>(out) + (size_t)j * 3u;
            __builtin_nontemporal_store(o0, dst);
            __builtin_nontemporal_store(o1, dst + 1);
            __builtin_nontemporal_store(o2, dst + 2);
        } else {
            uint32_t o[12];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint4 t = *reinterpret_cast<const uint4 *>(&tile[16u * j + 4u * g]);
                ego_pack4_rgb(rgb(t.x), rgb(t.y), rgb(t.z), rgb(t.w), o[3 * g], o[3 * g + 1], o[3 * g + 2]);
            }
            ego_u32x4 *const dst = reinterpret_cast<ego_u32x4 *>(out) + (size_t)j * 3u;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ego_u32x4 t;
                t.x = o[4 * k]; t.y = o[4 * k + 1]; t.z = o[4 * k + 2]; t.w = o[4 * k + 3];
                __builtin_nontemporal_store(t, dst + k);
            }
        }
    }
}

// Where band b of frame f starts in a slab of RGB24 frames W x H.
__device__ __forceinline__ uint8_t *ego_band_out(uint8_t *fb, uint32_t f, int32_t W, int32_t H, const EgoBand &b) {
    return fb + (size_t)f * 3u * (size_t)W * (size_t)H + (size_t)3u * (size_t)b.row0 * (size_t)W;
}

}  // namespace dg
