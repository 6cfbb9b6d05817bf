// plane_kernels.hip — gfx950 kernels of the depth planes, the label planes and a bundle's planes (include/doomgpu.h: dg_depth_*,
// dg_label_*, dg_bundle_*; the rule: plane_core.h).
//
// plane_tiles_body<DEPTH, LABELS, BOXES>  the one walk behind dg_depth_tiles, dg_label_tiles and dg_bundle_tiles<DEPTH, LABELS>: one
//                 workgroup (8 wavefronts) per (frame, 64-column strip, band of 128 rows), lane = column:
//                   * the waves share the strip's columns: wave w resolves spans w and w + 8 of every column (the column-invariant part
//                     of its mapper, once per workgroup) into LDS, [slot][word][lane] so that every access is one dword per lane on
//                     consecutive banks; a wall span's z or owner tag sits in word 3, and with DEPTH and LABELS a ninth word carries the
//                     tag next to z (36 KB, else 32 KB: four workgroups per CU either way) — one barrier;
//                   * wave w then takes rows band + w, + 8, ...: per row a lane walks its column's spans from the last to the first and
//                     stops at the first one that covers the row and is opaque there — the reference's "later Pixels::set wins" read
//                     backwards.  Only the covering span's other words are read, and only a masked wall, a sprite or a holey sky gathers
//                     a texel (the opacity byte); the one transparency test answers for distance, kind and label alike, and a flat
//                     divides only with DEPTH;
//                   * a column with more than PLANE_CAP spans reads the ones beyond from global memory and resolves them where they
//                     cover the row;
//                   * per row a wave stores 128 contiguous bytes of distance and 64 of kind (DEPTH), 128 of id and 64 of cls (LABELS).
//                     Every pixel of every requested plane is written (uncovered: far, 0; 0, 0);
//                   * boxes (BOXES): a lane keeps the map object it saw last, that object's pixel count and its first and last row over
//                     the rows its wave walks — pixels of other classes in between change nothing — and flushes an atomicAdd and four
//                     atomicMax into the frame's row of the box table (label_core.h: LabelRawBox), which the launch cleared, when
//                     ANOTHER object turns up.  What is held at the end of the band is combined across the wave first: per object one
//                     lane adds the sum and the maxima of all the lanes that hold it, five atomics per (wave, object) instead of per
//                     (lane, run) — measured, DESIGN.md §8i: 4 x on the whole kernel.  The updates are integer adds and maxima: neither
//                     their order nor the rows being every eighth nor the gaps inside an entry can show.
// dg_label_boxes  a label submission's boxes, from its planes: one workgroup (4 wavefronts) per (frame, 64-column strip, band of 128
//                 rows), lane = column, wave w = rows 32 w .. of the band: a lane walks its column piece top down and flushes one update
//                 per vertical run of one map-object id into the frame's row of the box table, which the launch cleared.
// No shading, no palette, no colour texel.  Plain C++: the compiler's IEEE divide, no inline assembly beyond raster_core.h's conversions.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "plane_core.h"
#include "plane_kernels.hpp"

namespace dg {

constexpr int PLANE_COLS = 64;         // columns per workgroup = lanes per wave
constexpr int PLANE_WAVES = 8;
constexpr int PLANE_THREADS = PLANE_WAVES * 64;
constexpr int PLANE_BAND = 128;        // rows per workgroup: 16 per wave, the spans resolved once for all of them
constexpr int PLANE_CAP = 16;          // spans per column staged in LDS (32 or 36 KB per workgroup: four workgroups = 32 waves per CU)
constexpr int BOX_WAVES = 4;
constexpr int BOX_THREADS = BOX_WAVES * 64;
constexpr int BOX_ROWS = PLANE_BAND / BOX_WAVES;   // rows of a band one wave of dg_label_boxes walks

// One entry's five updates (label_core.h: LabelRawBox): `pixels` more pixels in columns x0 .. x1, the last of their rows + 1 and H - the
// first of their rows.
__device__ __forceinline__ void box_update(LabelRawBox &e, uint32_t pixels, int32_t x0, int32_t x1, uint32_t y1p, uint32_t hy0, int32_t W) {
    atomicAdd(&e.w[0], pixels);
    atomicMax(&e.w[1], (uint32_t)(x1 + 1));
    atomicMax(&e.w[2], y1p);
    atomicMax(&e.w[3], (uint32_t)(W - x0));
    atomicMax(&e.w[4], hy0);
}

// (The parameters by value, as the kernels get them: taken by reference, dg_bundle_tiles<true, true> came out 64 B longer and measured
// 0.7 % slower — profiles/plane_kernels_refactor.md.)
template <bool DEPTH, bool LABELS, bool BOXES>
__device__ __forceinline__ void plane_tiles_body(RasterParams P, const uint32_t *owners, BundlePlanes out) {
    static_assert(LABELS || !BOXES, "boxes are made of labels");
    using Span = PlaneSpan<DEPTH, LABELS>;
    constexpr int WORDS = Span::WORDS;
    __shared__ uint32_t staged[PLANE_CAP][WORDS][PLANE_COLS];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int W = P.k.W, H = P.k.H;
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * PLANE_COLS + lane;
    const int y_begin = (int)blockIdx.y * PLANE_BAND, y_end = min(H, y_begin + PLANE_BAND);
    const DevFrame fr = P.frames[f];
    const bool live = x < W;
    uint32_t first = 0, n = 0;
    if (live) {
        const uint32_t *co = P.col_off + (size_t)f * (size_t)(W + 1) + (size_t)x;
        first = fr.span_base + co[0];
        n = co[1] - co[0];
    }
    const uint32_t n_staged = min(n, (uint32_t)PLANE_CAP);
    for (uint32_t j = (uint32_t)wave; j < n_staged; j += PLANE_WAVES) {
        const Span r = plane_resolve_span<DEPTH, LABELS>(P.spans[first + j], fr, P.walls, P.planes, owners, P.scene, P.k);
#pragma unroll
        for (int w = 0; w < WORDS; w++) staged[j][w][lane] = r.w[w];
    }
    __syncthreads();
    // With BOXES the lanes beyond the frame's last column stay: they have no spans and store nothing, and the wave's lanes combine
    // their boxes below.
    if (!BOXES && !live) return;
    int32_t run = -1, run_first = 0, run_last = 0;      // BOXES: the map object the lane saw last (-1: none yet), its first and last row so far
    uint32_t run_count = 0;                             // ... and its pixels so far
    LabelRawBox *const box_row = BOXES ? out.boxes + (size_t)f * (size_t)out.n_mobjs : nullptr;
    for (int y = y_begin + wave; y < y_end; y += PLANE_WAVES) {
        int32_t d = DEPTH_FAR;
        uint32_t kd = KIND_NONE, label = LABEL_NONE << 16;
        for (uint32_t j = n; j-- > 0;) {
            Span r;
            if (j < (uint32_t)PLANE_CAP) {
                r.w[0] = staged[j][0][lane];
                if (!plane_span_covers(r.w[0], y)) continue;
#pragma unroll
                for (int w = 1; w < WORDS; w++) r.w[w] = staged[j][w][lane];
            } else {
                const DevSpan sp = P.spans[first + j];
                if (y < (int)sp.ctop || y > (int)sp.cbot) continue;
                r = plane_resolve_span<DEPTH, LABELS>(sp, fr, P.walls, P.planes, owners, P.scene, P.k);
            }
            if (plane_span_writes<DEPTH>(r, P.scene, P.k, y, d, kd, label)) break;
        }
        if (BOXES && !live) continue;
        const size_t px = ((size_t)f * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
        if (DEPTH) {
            out.dist[px] = (int16_t)d;
            out.kind[px] = (uint8_t)kd;
        }
        if (LABELS) {
            out.id[px] = (uint16_t)label_index(label);
            out.cls[px] = (uint8_t)label_class(label);
        }
        if (BOXES) {
            const int32_t cur = label_class(label) == LABEL_MOBJ ? (int32_t)label_index(label) : -1;
            if (cur >= 0 && cur != run) {                   // another object: what the lane holds goes to the table
                if (run >= 0 && (uint32_t)run < out.n_mobjs)    // (the id is checked against the table before it is touched)
                    box_update(box_row[run], run_count, x, x, (uint32_t)(run_last + 1), (uint32_t)(H - run_first), W);
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
    if (BOXES) {
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
                const int x_hi = x + (63 - __clzll((long long)mask)) - leader;
                box_update(box_row[obj], count, x, x_hi, last1, first1, W);
            }
            todo &= ~mask;
        }
    }
}

__global__ __launch_bounds__(PLANE_THREADS) void dg_depth_tiles(RasterParams P, int16_t *dist, uint8_t *kind) {
    plane_tiles_body<true, false, false>(P, nullptr, BundlePlanes{dist, kind, nullptr, nullptr, nullptr, 0u});
}

__global__ __launch_bounds__(PLANE_THREADS) void dg_label_tiles(RasterParams P, const uint32_t *owners, uint16_t *id, uint8_t *cls) {
    plane_tiles_body<false, true, false>(P, owners, BundlePlanes{nullptr, nullptr, id, cls, nullptr, 0u});
}

template <bool DEPTH, bool LABELS>
__global__ __launch_bounds__(PLANE_THREADS) void dg_bundle_tiles(RasterParams P, const uint32_t *owners, BundlePlanes out) {
    plane_tiles_body<DEPTH, LABELS, LABELS>(P, owners, out);
}

__global__ __launch_bounds__(BOX_THREADS) void dg_label_boxes(const uint16_t *id, const uint8_t *cls, LabelRawBox *boxes, int W, int H, uint32_t n_mobjs) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int f = (int)blockIdx.z, x = (int)blockIdx.x * PLANE_COLS + lane;
    const int y_begin = (int)blockIdx.y * PLANE_BAND + wave * BOX_ROWS, y_end = min(H, y_begin + BOX_ROWS);
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

// Nothing to launch: the events are still recorded for whoever waits on them.
static hipError_t record_only(hipStream_t stream, std::initializer_list<hipEvent_t> events) {
    hipError_t e = hipSuccess;
    for (hipEvent_t ev : events)
        if (e == hipSuccess && ev) e = hipEventRecord(ev, stream);
    return e;
}

static dim3 plane_grid(const RasterParams &P) {
    return dim3((unsigned)((P.k.W + PLANE_COLS - 1) / PLANE_COLS), (unsigned)((P.k.H + PLANE_BAND - 1) / PLANE_BAND), (unsigned)P.n_frames);
}

static hipError_t clear_boxes(const RasterParams &P, LabelRawBox *boxes, uint32_t n_mobjs, hipStream_t stream) {
    return n_mobjs ? hipMemsetAsync(boxes, 0, (size_t)P.n_frames * (size_t)n_mobjs * sizeof(LabelRawBox), stream) : hipSuccess;
}

hipError_t launch_depth(const RasterParams &P, int16_t *dist, uint8_t *kind, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (P.n_frames <= 0) return record_only(stream, {start, stop});
    hipExtLaunchKernelGGL(dg_depth_tiles, plane_grid(P), dim3(PLANE_THREADS), 0, stream, start, stop, 0, P, dist, kind);
    return hipGetLastError();
}

hipError_t launch_labels(const RasterParams &P, const uint32_t *owners, uint16_t *id, uint8_t *cls, LabelRawBox *boxes, uint32_t n_mobjs,
                         hipStream_t stream, hipEvent_t start, hipEvent_t mid, hipEvent_t stop) {
    if (P.n_frames <= 0) return record_only(stream, {start, mid, stop});
    hipError_t e = clear_boxes(P, boxes, n_mobjs, stream);
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(dg_label_tiles, plane_grid(P), dim3(PLANE_THREADS), 0, stream, start, mid, 0, P, owners, id, cls);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipExtLaunchKernelGGL(dg_label_boxes, plane_grid(P), dim3(BOX_THREADS), 0, stream, nullptr, stop, 0, (const uint16_t *)id, (const uint8_t *)cls, boxes, P.k.W, P.k.H, n_mobjs);
    return hipGetLastError();
}

hipError_t launch_bundle(const RasterParams &P, const uint32_t *owners, const BundlePlanes &out, uint32_t what, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    const bool depth = (what & BUNDLE_DEPTH) != 0, labels = (what & BUNDLE_LABELS) != 0;
    if (P.n_frames <= 0 || (!depth && !labels)) return record_only(stream, {start, stop});
    if (labels) {
        const hipError_t e = clear_boxes(P, out.boxes, out.n_mobjs, stream);
        if (e != hipSuccess) return e;
    }
    const dim3 grid = plane_grid(P), block(PLANE_THREADS);
    if (depth && labels) hipExtLaunchKernelGGL((dg_bundle_tiles<true, true>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    else if (depth) hipExtLaunchKernelGGL((dg_bundle_tiles<true, false>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    else hipExtLaunchKernelGGL((dg_bundle_tiles<false, true>), grid, block, 0, stream, start, stop, 0, P, owners, out);
    return hipGetLastError();
}

}  // namespace dg
