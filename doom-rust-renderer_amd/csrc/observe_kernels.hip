// observe_kernels.hip — observation tensors (dg_observe_device): the box downscale of RGB24 frames or the representative
// distance of a box, clamped, mapped and narrowed (observe_core.h) into a strided (N, C, H, W) destination, in one pass over the source.
//
// dg_observe_rgb<PIECES> has the workgroup shape and the first two phases of dg_reduce (reduce_kernels.hip): one band of fy source rows
// of one frame x a run of whole output pixels;
//   1. the band's 16-bit sums per byte position into LDS (reduce_band.h), one barrier;
//   2. one lane per output element adds the fx column sums of its channel and divides (reduce_round);
//   3. DG_OBS_RGB stores that value through obs_put; DG_OBS_GRAY keeps the bytes in LDS and, after a second barrier, one lane per output
//      pixel stores the luma through obs_put.
//   The lane-to-element map of the RGB store (obs_item) is chosen per launch from the strides: with strides[3] == 1 consecutive lanes
//   take consecutive ox of one channel, otherwise the channels of consecutive pixels, so a wave's stores go to consecutive addresses
//   for NCHW and for channels-last alike.
// dg_observe_distance_nearest<PIECES>: phase 1 of dg_plane_nearest (reduce_band.h), then one lane per output pixel takes the minimum of
// its fx column keys and stores the distance in it.  dg_observe_distance_point: one lane per output pixel.
// All offsets are 64-bit; the only float arithmetic is obs_map's.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "observe_kernels.hpp"
#include "reduce_band.h"

namespace dg {

namespace {

struct ObserveParams {
    const void *src;
    void *dst;                     // element (0, 0, 0, 0) of this launch's first frame
    size_t src_frame;              // bytes (RGB24) / elements (distance) per source frame
    int64_t st[4];                 // strides in elements: frame, channel, row, column
    dg_obs_desc d;
    uint32_t W, H, oW, oH;
    uint32_t row_bytes;            // 3 W
    uint32_t px_per_wg;
    uint32_t rcp[4];               // reduce_rcp of the box sizes, as dg_reduce's
};

template <bool PIECES>
__global__ __launch_bounds__(REDUCE_LANES) void dg_observe_rgb(ObserveParams P) {
    __shared__ __attribute__((aligned(16))) uint16_t sums[REDUCE_SPAN];        // per byte position of the run: its sum over the band's rows
    __shared__ uint8_t rgb[(3u * reduce_px_per_wg(1u) + 15u) & ~15u];          // DG_OBS_GRAY: the run's rounded bytes
    const uint32_t tid = threadIdx.x, oy = blockIdx.y, fx = P.d.fx, fy = P.d.fy;
    const bool gray = P.d.source == DG_OBS_GRAY;
    uint32_t y0;
    const uint32_t ny = reduce_box(oy, fy, P.H, y0);
    const uint32_t ox0 = blockIdx.x * P.px_per_wg;
    const uint32_t np = min(P.px_per_wg, P.oW - ox0);                          // output pixels of this run
    const uint32_t b0 = 3u * fx * ox0;                                         // its source bytes within a row: [b0, b1)
    const uint32_t b1 = min(P.row_bytes, b0 + 3u * fx * np);
    const uint8_t *const rows = static_cast<const uint8_t *>(P.src) + (size_t)blockIdx.z * P.src_frame + (size_t)y0 * P.row_bytes;
    const uint32_t off0 = reduce_band_sums<PIECES>(sums, rows, P.row_bytes, ny, b0, b1, tid);
    __syncthreads();
    const uint32_t rcp_full = P.rcp[ny < fy ? 2 : 0], rcp_short = P.rcp[ny < fy ? 3 : 1];
    const int64_t at0 = (int64_t)blockIdx.z * P.st[0] + (int64_t)oy * P.st[2] + (int64_t)ox0 * P.st[3];
    const bool planar = !gray && P.st[3] == 1;
    for (uint32_t j = tid; j < 3u * np; j += REDUCE_LANES) {
        uint32_t p, c;
        obs_item(j, np, planar, p, c);
        uint32_t x0;
        const uint32_t nx = reduce_box(ox0 + p, fx, P.W, x0);
        const uint16_t *const e = sums + off0 + 3u * fx * p + c;
        uint32_t s = 0;
        for (uint32_t k = 0; k < nx; k++) s += e[3u * k];
        const uint32_t v = reduce_round(s, nx * ny, nx < fx ? rcp_short : rcp_full);
        if (gray) rgb[j] = (uint8_t)v;
        else obs_put(P.d, P.dst, at0 + (int64_t)c * P.st[1] + (int64_t)p * P.st[3], (int32_t)v);
    }
    if (gray) {
        __syncthreads();
        for (uint32_t p = tid; p < np; p += REDUCE_LANES)
            obs_put(P.d, P.dst, at0 + (int64_t)p * P.st[3], (int32_t)reduce_luma(rgb[3u * p], rgb[3u * p + 1u], rgb[3u * p + 2u]));
    }
}

template <bool PIECES>
__global__ __launch_bounds__(PLANE_REDUCE_LANES) void dg_observe_distance_nearest(ObserveParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t cols[PLANE_REDUCE_SPAN];  // per source column of the run: its key over the band's rows
    const uint32_t tid = threadIdx.x, oy = blockIdx.y, fx = P.d.fx;
    uint32_t y0;
    const uint32_t ny = reduce_box(oy, P.d.fy, P.H, y0);
    const uint32_t ox0 = blockIdx.x * P.px_per_wg;
    const uint32_t np = min(P.px_per_wg, P.oW - ox0);                          // output pixels of this run
    const uint32_t c0 = fx * ox0;                                              // its source columns: [c0, c1)
    const uint32_t c1 = min(P.W, c0 + fx * np);
    const int16_t *const rows = static_cast<const int16_t *>(P.src) + (size_t)blockIdx.z * P.src_frame + (size_t)y0 * P.W;
    const uint32_t off0 = plane_band_keys<PIECES>(cols, rows, P.W, ny, c0, c1, tid);
    __syncthreads();
    const int64_t at0 = (int64_t)blockIdx.z * P.st[0] + (int64_t)oy * P.st[2] + (int64_t)ox0 * P.st[3];
    for (uint32_t p = tid; p < np; p += PLANE_REDUCE_LANES) {
        uint32_t x0;
        const uint32_t nx = reduce_box(ox0 + p, fx, P.W, x0);
        const uint32_t *const e = cols + off0 + fx * p;
        uint32_t best = PLANE_KEY_NONE;
        for (uint32_t rx = 0; rx < nx; rx++) best = min(best, plane_box_key(e[rx], rx));
        obs_put(P.d, P.dst, at0 + (int64_t)p * P.st[3], (int32_t)plane_key_distance(best));
    }
}

__global__ __launch_bounds__(PLANE_REDUCE_LANES) void dg_observe_distance_point(ObserveParams P) {
    const uint32_t ox = blockIdx.x * PLANE_REDUCE_LANES + threadIdx.x, oy = blockIdx.y;
    if (ox >= P.oW) return;
    const int16_t *const frame = static_cast<const int16_t *>(P.src) + (size_t)blockIdx.z * P.src_frame;
    const int16_t v = frame[(size_t)plane_point(oy, P.d.fy, P.H) * P.W + plane_point(ox, P.d.fx, P.W)];
    obs_put(P.d, P.dst, (int64_t)blockIdx.z * P.st[0] + (int64_t)oy * P.st[2] + (int64_t)ox * P.st[3], (int32_t)v);
}

}  // namespace

hipError_t launch_observe(const void *src, int W, int H, int n_frames, const dg_obs_desc &d, void *dst, const int64_t strides[4], hipStream_t stream,
                          hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    const bool colour = d.source != DG_OBS_DISTANCE, nearest = !colour && d.rule == DG_PLANE_NEAREST;
    ObserveParams P{};
    P.d = d;
    P.W = (uint32_t)W; P.H = (uint32_t)H;
    P.oW = reduce_out_dim(P.W, d.fx); P.oH = reduce_out_dim(P.H, d.fy);
    P.row_bytes = 3u * P.W;
    for (int i = 0; i < 4; i++) P.st[i] = strides[i];
    bool pieces;
    uint32_t runs;
    if (colour) {
        P.px_per_wg = reduce_px_per_wg(d.fx);
        P.src_frame = (size_t)P.row_bytes * (size_t)P.H;
        uint32_t lo;
        const uint32_t nx_last = reduce_box(P.oW - 1u, d.fx, P.W, lo), ny_last = reduce_box(P.oH - 1u, d.fy, P.H, lo);
        P.rcp[0] = reduce_rcp(d.fx * d.fy); P.rcp[1] = reduce_rcp(nx_last * d.fy);
        P.rcp[2] = reduce_rcp(d.fx * ny_last); P.rcp[3] = reduce_rcp(nx_last * ny_last);
        pieces = P.row_bytes % 16u == 0u && reinterpret_cast<uintptr_t>(src) % 16u == 0u;
        runs = (P.oW + P.px_per_wg - 1u) / P.px_per_wg;
    } else {
        P.px_per_wg = plane_reduce_px_per_wg(d.fx);
        P.src_frame = (size_t)P.W * (size_t)P.H;
        pieces = P.W % 8u == 0u && reinterpret_cast<uintptr_t>(src) % 16u == 0u;
        runs = nearest ? (P.oW + P.px_per_wg - 1u) / P.px_per_wg : (P.oW + PLANE_REDUCE_LANES - 1u) / PLANE_REDUCE_LANES;
    }
    const size_t src_step = P.src_frame * (colour ? 1u : sizeof(int16_t)), dst_step = (size_t)strides[0] * obs_element_bytes(d.dtype);
    constexpr int kMaxZ = 65535;                               // frames per launch: the grid's z extent
    for (int f0 = 0; f0 < n_frames; f0 += kMaxZ) {
        const int nf = std::min(kMaxZ, n_frames - f0);
        P.src = static_cast<const uint8_t *>(src) + (size_t)f0 * src_step;
        P.dst = static_cast<uint8_t *>(dst) + (size_t)f0 * dst_step;
        const dim3 grid(runs, P.oH, (unsigned)nf);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == n_frames ? stop : nullptr;
        if (colour && pieces) hipExtLaunchKernelGGL(dg_observe_rgb<true>, grid, dim3(REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else if (colour) hipExtLaunchKernelGGL(dg_observe_rgb<false>, grid, dim3(REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else if (!nearest) hipExtLaunchKernelGGL(dg_observe_distance_point, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else if (pieces) hipExtLaunchKernelGGL(dg_observe_distance_nearest<true>, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else hipExtLaunchKernelGGL(dg_observe_distance_nearest<false>, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
