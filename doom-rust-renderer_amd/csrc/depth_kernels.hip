// depth_kernels.hip — gfx950 kernel of the depth / surface-kind frame (include/doomgpu.h: dg_depth_*; arithmetic: depth_core.h).
//
// dg_depth_tiles  one workgroup (8 wavefronts) per (frame, 64-column strip, band of 128 rows), lane = column:
//                   * the waves share the strip's columns: wave w resolves spans w and w + 8 of every column (the column-invariant part
//                     of its mapper, once per workgroup) into LDS, [slot][word][lane] so that every access is one dword per lane on
//                     consecutive banks — one barrier;
//                   * wave w then takes rows band + w, + 8, ...: per row a lane walks its column's spans from the last to the first and
//                     stops at the first one that covers the row and is opaque there — the reference's "later Pixels::set wins" read
//                     backwards.  Only the covering span's other words are read, and only a masked wall, a sprite or a holey sky gathers
//                     a texel (the opacity byte);
//                   * a column with more than DEPTH_CAP spans reads the ones beyond from global memory and resolves them where they
//                     cover the row;
//                   * a wave stores 128 contiguous bytes of distance and 64 of kind per row.  Every pixel is written (uncovered: far, 0).
// No shading, no palette, no colour texel.  Plain C++: the compiler's IEEE divide, no inline assembly beyond raster_core.h's conversions.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "depth_core.h"
#include "depth_kernels.hpp"

namespace dg {

constexpr int DEPTH_COLS = 64;         // columns per workgroup = lanes per wave
constexpr int DEPTH_WAVES = 8;
constexpr int DEPTH_THREADS = DEPTH_WAVES * 64;
constexpr int DEPTH_BAND = 128;        // rows per workgroup: 16 per wave, the spans resolved once for all of them
constexpr int DEPTH_CAP = 16;          // spans per column staged in LDS (32 KB per workgroup: four workgroups = 32 waves per CU)

__global__ __launch_bounds__(DEPTH_THREADS) void dg_depth_tiles(RasterParams P, int16_t *dist, uint8_t *kind) {
    __shared__ uint32_t staged[DEPTH_CAP][8][DEPTH_COLS];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int W = P.k.W, H = P.k.H;
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * DEPTH_COLS + lane;
    const int y_begin = (int)blockIdx.y * DEPTH_BAND, y_end = min(H, y_begin + DEPTH_BAND);
    const DevFrame fr = P.frames[f];
    const bool live = x < W;
    uint32_t first = 0, n = 0;
    if (live) {
        const uint32_t *co = P.col_off + (size_t)f * (size_t)(W + 1) + (size_t)x;
        first = fr.span_base + co[0];
        n = co[1] - co[0];
    }
    const uint32_t n_staged = min(n, (uint32_t)DEPTH_CAP);
    for (uint32_t j = (uint32_t)wave; j < n_staged; j += DEPTH_WAVES) {
        const DevRSpan r = depth_resolve_span(P.spans[first + j], fr, P.walls, P.planes, P.scene, P.k);
#pragma unroll
        for (int w = 0; w < 8; w++) staged[j][w][lane] = r.w[w];
    }
    __syncthreads();
    if (!live) return;
    for (int y = y_begin + wave; y < y_end; y += DEPTH_WAVES) {
        int32_t d = DEPTH_FAR;
        uint32_t kd = KIND_NONE;
        for (uint32_t j = n; j-- > 0;) {
            DevRSpan r;
            if (j < (uint32_t)DEPTH_CAP) {
                r.w[0] = staged[j][0][lane];
                if (!depth_span_covers(r.w[0], y)) continue;
#pragma unroll
                for (int w = 1; w < 8; w++) r.w[w] = staged[j][w][lane];
            } else {
                const DevSpan sp = P.spans[first + j];
                if (y < (int)sp.ctop || y > (int)sp.cbot) continue;
                r = depth_resolve_span(sp, fr, P.walls, P.planes, P.scene, P.k);
            }
            if (depth_span_writes(r, P.scene, P.k, y, d, kd)) break;
        }
        const size_t px = ((size_t)f * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
        dist[px] = (int16_t)d;
        kind[px] = (uint8_t)kd;
    }
}

hipError_t launch_depth(const RasterParams &P, int16_t *dist, uint8_t *kind, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (P.n_frames <= 0) {                                  // nothing to launch: the events are still recorded for whoever waits on them
        hipError_t e = hipSuccess;
        if (start) e = hipEventRecord(start, stream);
        if (e == hipSuccess && stop) e = hipEventRecord(stop, stream);
        return e;
    }
    const dim3 grid((unsigned)((P.k.W + DEPTH_COLS - 1) / DEPTH_COLS), (unsigned)((P.k.H + DEPTH_BAND - 1) / DEPTH_BAND), (unsigned)P.n_frames);
    hipExtLaunchKernelGGL(dg_depth_tiles, grid, dim3(DEPTH_THREADS), 0, stream, start, stop, 0, P, dist, kind);
    return hipGetLastError();
}

}  // namespace dg
