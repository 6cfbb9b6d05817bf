// label_kernels.hip — gfx950 kernels of the object-label frame (include/doomgpu.h: dg_label_*; rules: label_core.h).
//
// dg_label_tiles  dg_depth_tiles' decomposition (depth_kernels.hip) with another payload: one workgroup (8 wavefronts) per
//                 (frame, 64-column strip, band of 128 rows), lane = column:
//                   * wave w resolves spans w and w + 8 of every column into LDS, [slot][word][lane] — one dword per lane on consecutive
//                     banks for every access — with the owner tag of a wall span's draw record in word 3; one barrier;
//                   * wave w then takes rows band + w, + 8, ...: per row a lane walks its column's spans from the last to the first and
//                     stops at the first one that covers the row and is opaque there.  Only a masked wall, a sprite or a holey sky gathers
//                     a texel (the opacity byte); a flat writes its class without evaluating anything;
//                   * a column with more than LABEL_CAP spans reads the ones beyond from global memory and resolves them where they cover
//                     the row;
//                   * a wave stores 128 contiguous bytes of id and 64 of cls per row.  Every pixel is written (uncovered: 0, 0).
// dg_label_boxes  one workgroup (4 wavefronts) per (frame, 64-column strip, band of 128 rows), lane = column, wave w = rows 32 w .. of the
//                 band: a lane walks its column piece top down and flushes one update per vertical run of one map-object id — an
//                 atomicAdd of the run's length and four atomicMax (label_core.h: LabelRawBox) — into the frame's row of the box table,
//                 which the launch cleared.  Integer updates: their order cannot show.
// Plain C++; no inline assembly beyond raster_core.h's conversions.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "label_core.h"
#include "label_kernels.hpp"

namespace dg {

constexpr int LABEL_COLS = 64;         // columns per workgroup = lanes per wave
constexpr int LABEL_WAVES = 8;
constexpr int LABEL_THREADS = LABEL_WAVES * 64;
constexpr int LABEL_BAND = 128;        // rows per workgroup
constexpr int LABEL_CAP = 16;          // spans per column staged in LDS (32 KB per workgroup)
constexpr int BOX_WAVES = 4;
constexpr int BOX_THREADS = BOX_WAVES * 64;
constexpr int BOX_ROWS = LABEL_BAND / BOX_WAVES;   // rows of a band one wave of dg_label_boxes walks

__global__ __launch_bounds__(LABEL_THREADS) void dg_label_tiles(RasterParams P, const uint32_t *owners, uint16_t *id, uint8_t *cls) {
    __shared__ uint32_t staged[LABEL_CAP][8][LABEL_COLS];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int W = P.k.W, H = P.k.H;
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * LABEL_COLS + lane;
    const int y_begin = (int)blockIdx.y * LABEL_BAND, y_end = min(H, y_begin + LABEL_BAND);
    const DevFrame fr = P.frames[f];
    const bool live = x < W;
    uint32_t first = 0, n = 0;
    if (live) {
        const uint32_t *co = P.col_off + (size_t)f * (size_t)(W + 1) + (size_t)x;
        first = fr.span_base + co[0];
        n = co[1] - co[0];
    }
    const uint32_t n_staged = min(n, (uint32_t)LABEL_CAP);
    for (uint32_t j = (uint32_t)wave; j < n_staged; j += LABEL_WAVES) {
        const DevRSpan r = label_resolve_span(P.spans[first + j], fr, P.walls, owners, P.scene, P.k);
#pragma unroll
        for (int w = 0; w < 8; w++) staged[j][w][lane] = r.w[w];
    }
    __syncthreads();
    if (!live) return;
    for (int y = y_begin + wave; y < y_end; y += LABEL_WAVES) {
        uint32_t label = LABEL_NONE << 16;
        for (uint32_t j = n; j-- > 0;) {
            DevRSpan r;
            if (j < (uint32_t)LABEL_CAP) {
                r.w[0] = staged[j][0][lane];
                if (!label_span_covers(r.w[0], y)) continue;
#pragma unroll
                for (int w = 1; w < 8; w++) r.w[w] = staged[j][w][lane];
            } else {
                const DevSpan sp = P.spans[first + j];
                if (y < (int)sp.ctop || y > (int)sp.cbot) continue;
                r = label_resolve_span(sp, fr, P.walls, owners, P.scene, P.k);
            }
            if (label_span_writes(r, P.scene, P.k, y, label)) break;
        }
        const size_t px = ((size_t)f * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
        id[px] = (uint16_t)label_index(label);
        cls[px] = (uint8_t)label_class(label);
    }
}

__global__ __launch_bounds__(BOX_THREADS) void dg_label_boxes(const uint16_t *id, const uint8_t *cls, LabelRawBox *boxes, int W, int H, uint32_t n_mobjs) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * LABEL_COLS + lane;
    const int y_begin = (int)blockIdx.y * LABEL_BAND + wave * BOX_ROWS, y_end = min(H, y_begin + BOX_ROWS);
    if (x >= W) return;
    LabelRawBox *const row = boxes + (size_t)f * (size_t)n_mobjs;
    const size_t col = (size_t)f * (size_t)H * (size_t)W + (size_t)x;
    int32_t run = -1, run_top = 0;                  // the map object of the run the walk is in (-1: none) and the run's first row
    for (int y = y_begin; y <= y_end; y++) {        // (one step past the piece closes its last run)
        int32_t cur = -1;
        if (y < y_end) {
            const size_t px = col + (size_t)y * (size_t)W;
            if (cls[px] == (uint8_t)LABEL_MOBJ) cur = (int32_t)id[px];
        }
        if (cur == run) continue;
        if (run >= 0 && (uint32_t)run < n_mobjs) {
            uint32_t *const b = row[run].w;
            atomicAdd(&b[0], (uint32_t)(y - run_top));
            atomicMax(&b[1], (uint32_t)(x + 1));
            atomicMax(&b[2], (uint32_t)y);            // (y - 1) + 1: the run's last row
            atomicMax(&b[3], (uint32_t)(W - x));
            atomicMax(&b[4], (uint32_t)(H - run_top));
        }
        run = cur;
        run_top = y;
    }
}

hipError_t launch_labels(const RasterParams &P, const uint32_t *owners, uint16_t *id, uint8_t *cls, LabelRawBox *boxes, uint32_t n_mobjs,
                         hipStream_t stream, hipEvent_t start, hipEvent_t mid, hipEvent_t stop) {
    if (P.n_frames <= 0) {                                  // nothing to launch: the events are still recorded for whoever waits on them
        hipError_t e = hipSuccess;
        for (hipEvent_t ev : {start, mid, stop})
            if (e == hipSuccess && ev) e = hipEventRecord(ev, stream);
        return e;
    }
    if (n_mobjs) {
        const hipError_t e = hipMemsetAsync(boxes, 0, (size_t)P.n_frames * (size_t)n_mobjs * sizeof(LabelRawBox), stream);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((P.k.W + LABEL_COLS - 1) / LABEL_COLS), (unsigned)((P.k.H + LABEL_BAND - 1) / LABEL_BAND), (unsigned)P.n_frames);
    hipExtLaunchKernelGGL(dg_label_tiles, grid, dim3(LABEL_THREADS), 0, stream, start, mid, 0, P, owners, id, cls);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(dg_label_boxes, grid, dim3(BOX_THREADS), 0, stream, nullptr, stop, 0, (const uint16_t *)id, (const uint8_t *)cls, boxes, P.k.W, P.k.H, n_mobjs);
    return hipGetLastError();
}

}  // namespace dg
