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

namespace dg {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxY = 65535;                              // frames per launch: the grid's y extent

template <uint32_t TILE, int PX>
__global__ void __launch_bounds__(kThreads) dg_ego_tiles(EgoParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[TILE];
    __shared__ MapSeg list[EGO_CHUNK];
    __shared__ uint32_t n_list[2];                        // chunk c appends through n_list[c & 1]; the other one is cleared meanwhile
    const uint32_t tid = threadIdx.x, f = blockIdx.y;
    const int32_t W = p.W, H = p.H;
    const uint32_t band_rows = ego_band_rows((uint32_t)W);
    const int32_t row0 = (int32_t)(blockIdx.x * band_rows);
    if (row0 >= H) return;                                // (the grid has ego_bands bands: never)
    const int32_t rows = min((int32_t)band_rows, H - row0);
    const uint32_t px = (uint32_t)rows * (uint32_t)W;
    if (px > TILE) return;                                // (the launcher picks TILE so: never)
    for (uint32_t i = 4u * tid; i < px; i += 4u * kThreads)     // i + 3 < TILE: both are multiples of 4
        *reinterpret_cast<uint4 *>(&tile[i]) = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 2u) n_list[tid] = 0u;
    const EgoView v = p.views[f];
    const uint32_t *const mask = p.masks ? p.masks + (size_t)f * p.mask_words : nullptr;
    const bool rotate = p.rotate != 0u;
    __syncthreads();
    uint32_t parity = 0u;
    for (uint32_t base = 0; base < p.n_lines; base += EGO_CHUNK, parity ^= 1u) {
        const uint32_t l = base + tid;
        if (l < p.n_lines) {
            const uint32_t w = p.words[l];
            if ((w & EGO_DRAWN) && (!mask || ((mask[l >> 5] >> (l & 31u)) & 1u))) {
                const MapSeg s = ego_band_seg(p.lines[l], w & ~EGO_DRAWN, v, p.scale, rotate, W, H, row0, rows);
                if (s.count > 0) {
                    const uint32_t at = atomicAdd(&n_list[parity], 1u);
                    if (at < EGO_CHUNK) list[at] = s;     // (a chunk has EGO_CHUNK lines: always)
                }
            }
        }
        __syncthreads();
        const uint32_t n = min(n_list[parity], EGO_CHUNK);
        if (tid == 0u) n_list[parity ^ 1u] = 0u;          // the next chunk appends only after the barrier below
        for (uint32_t e = tid / kWave; e < n; e += kThreads / kWave) {
            const MapSeg s = list[e];
            for (int32_t k = (int32_t)(tid % kWave); k < s.count; k += kWave) {
                int32_t x, y;
                map_seg_point(s, (int64_t)s.first + k, x, y);
                if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)rows) atomicMax(&tile[(uint32_t)y * (uint32_t)W + (uint32_t)x], s.rgb);
            }
        }
        __syncthreads();
    }
    if (p.arrow) {
        for (uint32_t a = 0; a < 3u; a++) {
            const MapSeg s = p.arrow[(size_t)3u * f + a];
            int32_t lo, hi;
            ego_seg_rows(s, lo, hi);
            if (s.count <= 0 || hi < row0 || lo >= row0 + rows) continue;
            for (int32_t k = (int32_t)tid; k < s.count; k += kThreads) {
                int32_t x, y;
                map_seg_point(s, (int64_t)s.first + k, x, y);
                y -= row0;
                if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)rows) atomicMax(&tile[(uint32_t)y * (uint32_t)W + (uint32_t)x], EGO_ARROW_VALUE);
            }
        }
        __syncthreads();
    }
    uint8_t *const out = p.fb + (size_t)f * 3u * (size_t)W * (size_t)H + (size_t)3u * (size_t)row0 * (size_t)W;
    const uint32_t n_items = px / PX;                     // PX divides px (the launcher picks PX so)
    for (uint32_t j = tid; j < n_items; j += kThreads) {
        if constexpr (PX == 1) {
            const uint32_t rgb = ego_value_rgb(tile[j]);
            uint8_t *const o = out + 3u * (size_t)j;
            o[0] = (uint8_t)rgb; o[1] = (uint8_t)(rgb >> 8); o[2] = (uint8_t)(rgb >> 16);
        } else if constexpr (PX == 4) {
            const uint4 t = *reinterpret_cast<const uint4 *>(&tile[4u * j]);
            uint32_t o0, o1, o2;
            ego_pack4(t.x, t.y, t.z, t.w, o0, o1, o2);
            uint32_t *const dst = reinterpret_cast<uint32_t *>(out) + (size_t)j * 3u;
            __builtin_nontemporal_store(o0, dst);
            __builtin_nontemporal_store(o1, dst + 1);
            __builtin_nontemporal_store(o2, dst + 2);
        } else {
            uint32_t o[12];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint4 t = *reinterpret_cast<const uint4 *>(&tile[16u * j + 4u * g]);
                ego_pack4(t.x, t.y, t.z, t.w, o[3 * g], o[3 * g + 1], o[3 * g + 2]);
            }
            u32x4 *const dst = reinterpret_cast<u32x4 *>(out) + (size_t)j * 3u;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                u32x4 t;
                t.x = o[4 * k]; t.y = o[4 * k + 1]; t.z = o[4 * k + 2]; t.w = o[4 * k + 3];
                __builtin_nontemporal_store(t, dst + k);
            }
        }
    }
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
