// bundle_kernels.hip — gfx950 kernel of a bundle submission (include/doomgpu.h: dg_bundle_*; rules: bundle_core.h).
//
// dg_bundle_tiles<DEPTH, LABELS>  the depth planes, the label planes and the per-object boxes of the same spans out of ONE walk.
//                 dg_depth_tiles' decomposition (depth_kernels.hip): one workgroup (8 wavefronts) per (frame, 64-column
//                 strip, band of 128 rows), lane = column:
//                   * wave w resolves spans w and w + 8 of every column into LDS, [slot][word][lane] — one dword per lane on consecutive
//                     banks for every access; with LABELS a ninth word carries a wall span's owner tag next to its z (36 KB, else 32 KB:
//                     four workgroups per CU either way); one barrier;
//                   * wave w then takes rows band + w, + 8, ...: per row a lane walks its column's spans from the last to the first and
//                     stops at the first one that covers the row and is opaque there; the one transparency test answers for distance,
//                     kind and label alike, and a flat divides only with DEPTH;
//                   * a column with more than BUNDLE_CAP spans reads the ones beyond from global memory and resolves them where they
//                     cover the row;
//                   * per row a wave stores 128 contiguous bytes of distance and 64 of kind (DEPTH), 128 of id and 64 of cls (LABELS).
//                     Every pixel of every requested plane is written;
//                   * boxes (LABELS): a lane keeps the map object it saw last, that object's pixel count and its first and last row over
//                     the rows its wave walks — pixels of other classes in between change nothing — and flushes an atomicAdd and four
//                     atomicMax into the frame's row of the box table (label_core.h: LabelRawBox), which the launch cleared, when
//                     ANOTHER object turns up.  What is held at the end of the band is combined across the wave first: per object one
//                     lane adds the sum and the maxima of all the lanes that hold it, five atomics per (wave, object) instead of per
//                     (lane, run) — measured, DESIGN.md §8i: 4 x on the whole kernel.  The updates are integer adds and maxima: neither
//                     their order nor the rows being every eighth nor the gaps inside an entry can show.
// Plain C++; no inline assembly beyond raster_core.h's conversions.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "bundle_core.h"
#include "bundle_kernels.hpp"

namespace dg {

constexpr int BUNDLE_COLS = 64;        // columns per workgroup = lanes per wave
constexpr int BUNDLE_WAVES = 8;
constexpr int BUNDLE_THREADS = BUNDLE_WAVES * 64;
constexpr int BUNDLE_BAND = 128;       // rows per workgroup: 16 per wave, the spans resolved once for all of them
constexpr int BUNDLE_CAP = 16;         // spans per column staged in LDS

// What a lane holds of one map object, into the frame's box row.  The id is checked against the table before it is touched.
__device__ __forceinline__ void bundle_box_flush(LabelRawBox *row, uint32_t n_mobjs, int32_t run, uint32_t count, int32_t y_first, int32_t y_last,
                                                 int32_t x, int32_t W, int32_t H) {
    if (run < 0 || (uint32_t)run >= n_mobjs) return;
    uint32_t *const b = row[run].w;
    atomicAdd(&b[0], count);
    atomicMax(&b[1], (uint32_t)(x + 1));
    atomicMax(&b[2], (uint32_t)(y_last + 1));
    atomicMax(&b[3], (uint32_t)(W - x));
    atomicMax(&b[4], (uint32_t)(H - y_first));
}

template <bool DEPTH, bool LABELS>
__global__ __launch_bounds__(BUNDLE_THREADS) void dg_bundle_tiles(RasterParams P, const uint32_t *owners, BundlePlanes out) {
    constexpr int WORDS = LABELS ? BUNDLE_WORDS : 8;
    __shared__ uint32_t staged[BUNDLE_CAP][WORDS][BUNDLE_COLS];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int W = P.k.W, H = P.k.H;
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * BUNDLE_COLS + lane;
    const int y_begin = (int)blockIdx.y * BUNDLE_BAND, y_end = min(H, y_begin + BUNDLE_BAND);
    const DevFrame fr = P.frames[f];
    const bool live = x < W;
    uint32_t first = 0, n = 0;
    if (live) {
        const uint32_t *co = P.col_off + (size_t)f * (size_t)(W + 1) + (size_t)x;
        first = fr.span_base + co[0];
        n = co[1] - co[0];
    }
    const uint32_t n_staged = min(n, (uint32_t)BUNDLE_CAP);
    for (uint32_t j = (uint32_t)wave; j < n_staged; j += BUNDLE_WAVES) {
        const BundleRSpan r = bundle_resolve_span<DEPTH, LABELS>(P.spans[first + j], fr, P.walls, P.planes, owners, P.scene, P.k);
#pragma unroll
        for (int w = 0; w < WORDS; w++) staged[j][w][lane] = r.w[w];
    }
    __syncthreads();
    // (lanes beyond the frame's last column stay: they have no spans and store nothing, and the wave's lanes combine their boxes below)
    int32_t run = -1, run_first = 0, run_last = 0;      // the map object the lane saw last (-1: none yet), its first and last row so far
    uint32_t run_count = 0;                             // ... and its pixels so far
    LabelRawBox *const box_row = LABELS ? out.boxes + (size_t)f * (size_t)out.n_mobjs : nullptr;
    for (int y = y_begin + wave; y < y_end; y += BUNDLE_WAVES) {
        int32_t d = DEPTH_FAR;
        uint32_t kd = KIND_NONE, label = LABEL_NONE << 16;
        for (uint32_t j = n; j-- > 0;) {
            BundleRSpan r;
            if (j < (uint32_t)BUNDLE_CAP) {
                r.w[0] = staged[j][0][lane];
                if (!bundle_span_covers(r.w[0], y)) continue;
#pragma unroll
                for (int w = 1; w < WORDS; w++) r.w[w] = staged[j][w][lane];
                if (!LABELS) r.w[8] = 0;
            } else {
                const DevSpan sp = P.spans[first + j];
                if (y < (int)sp.ctop || y > (int)sp.cbot) continue;
                r = bundle_resolve_span<DEPTH, LABELS>(sp, fr, P.walls, P.planes, owners, P.scene, P.k);
            }
            if (bundle_span_writes<DEPTH>(r, P.scene, P.k, y, d, kd, label)) break;
        }
        if (!live) continue;
        const size_t px = ((size_t)f * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
        if (DEPTH) {
            out.dist[px] = (int16_t)d;
            out.kind[px] = (uint8_t)kd;
        }
        if (LABELS) {
            out.id[px] = (uint16_t)label_index(label);
            out.cls[px] = (uint8_t)label_class(label);
            const int32_t cur = label_class(label) == LABEL_MOBJ ? (int32_t)label_index(label) : -1;
            if (cur >= 0 && cur != run) {                   // another object: what the lane holds goes to the table
                bundle_box_flush(box_row, out.n_mobjs, run, run_count, run_first, run_last, x, W, H);
                run = cur;
                run_count = 0;
                run_first = y;
            }
            if (cur >= 0) {
                run_count++;
                run_last = y;
            }
        }
    }
    // What the lanes still hold, one object at a time: the lanes that hold the first remaining lane's object reduce their entries across
    // the wave and the first of them updates the table once for all.
    if (LABELS) {
        unsigned long long todo = __ballot(run >= 0 && (uint32_t)run < out.n_mobjs);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t obj = __shfl(run, leader);
            const bool mine = run == obj;
            const unsigned long long mask = __ballot(mine);
            uint32_t count = mine ? run_count : 0u, last1 = mine ? (uint32_t)(run_last + 1) : 0u, first1 = mine ? (uint32_t)(H - run_first) : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                count += __shfl_xor(count, o);
                last1 = max(last1, __shfl_xor(last1, o));
                first1 = max(first1, __shfl_xor(first1, o));
            }
            if (lane == leader) {
                uint32_t *const b = box_row[obj].w;
                const int x_hi = x + (63 - __clzll((long long)mask)) - leader;
                atomicAdd(&b[0], count);
                atomicMax(&b[1], (uint32_t)(x_hi + 1));
                atomicMax(&b[2], last1);
                atomicMax(&b[3], (uint32_t)(W - x));
                atomicMax(&b[4], first1);
            }
            todo &= ~mask;
        }
    }
}

hipError_t launch_bundle(const RasterParams &P, const uint32_t *owners, const BundlePlanes &out, uint32_t what, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    const bool depth = (what & BUNDLE_DEPTH) != 0, labels = (what & BUNDLE_LABELS) != 0;
    if (P.n_frames <= 0 || (!depth && !labels)) {           // nothing to launch: the events are still recorded for whoever waits on them
        hipError_t e = hipSuccess;
        if (start) e = hipEventRecord(start, stream);
        if (e == hipSuccess && stop) e = hipEventRecord(stop, stream);
        return e;
    }
    if (labels && out.n_mobjs) {
        const hipError_t e = hipMemsetAsync(out.boxes, 0, (size_t)P.n_frames * (size_t)out.n_mobjs * sizeof(LabelRawBox), stream);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((P.k.W + BUNDLE_COLS - 1) / BUNDLE_COLS), (unsigned)((P.k.H + BUNDLE_BAND - 1) / BUNDLE_BAND), (unsigned)P.n_frames);
    const dim3 block(BUNDLE_THREADS);
    if (depth && labels) hipExtLaunchKernelGGL((dg_bundle_tiles<true, true>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    else if (depth) hipExtLaunchKernelGGL((dg_bundle_tiles<true, false>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    else hipExtLaunchKernelGGL((dg_bundle_tiles<false, true>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    return hipGetLastError();
}

}  // namespace dg
