// plane_reduce_kernels.hip — reduced-size depth and label planes (dg_reduce_planes_device, dg_readback_planes_reduced*):
// per box ONE representative source pixel, whose distance, kind, id and cls every requested output takes unchanged.
//
// dg_plane_nearest (DG_PLANE_NEAREST) is a streaming arg-min over the distance plane and a gather from the others.  One workgroup = one
// band of fy source rows of one frame x a run of whole output pixels (plane_reduce_px_per_wg), the shape of dg_reduce:
//   1. (reduce_band.h) every lane keeps, per source column it reads, the minimum over the band's rows of plane_col_key (distance, row) in registers and
//      puts it in LDS; dg_plane_nearest<true>: one 16-byte piece of 8 distances per lane and row, the pieces of a row consecutive and
//      16-byte aligned (2 W % 16 == 0, aligned base), so the run starts up to 7 columns in front of its first pixel;
//      dg_plane_nearest<false> (any width, any 2-byte aligned base): the lanes of a wave read 64 consecutive distances per load, 8 loads
//      per row;
//   2. after one barrier, one lane per output pixel takes the minimum of its fx column keys with the column appended (plane_box_key),
//      decodes the representative's row and column from it, reads kind / id / cls there and stores every requested output.
// dg_plane_point (DG_PLANE_POINT) needs no first phase: one lane per output pixel.
// No float arithmetic, plain loads and stores.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "plane_reduce_kernels.hpp"
#include "reduce_band.h"

namespace dg {

namespace {

struct PlaneReduceParams {
    PlaneReduceSrc src;
    PlaneReduceDst dst;
    size_t src_px, dst_px;         // elements per source / reduced frame of one plane
    uint32_t W, H, fx, fy, oW, oH;
    uint32_t px_per_wg;
};

// Output pixel (ox, oy) of frame f takes source pixel (x, y); d: its distance when the caller has it already.
template <bool HAVE_D>
__device__ __forceinline__ void plane_take(const PlaneReduceParams &P, uint32_t f, uint32_t ox, uint32_t oy, uint32_t x, uint32_t y, int16_t d) {
    const size_t s = (size_t)f * P.src_px + (size_t)y * P.W + x, o = (size_t)f * P.dst_px + (size_t)oy * P.oW + ox;
    if (P.dst.distance) P.dst.distance[o] = HAVE_D ? d : P.src.distance[s];
    if (P.dst.kind) P.dst.kind[o] = P.src.kind[s];
    if (P.dst.id) P.dst.id[o] = P.src.id[s];
    if (P.dst.cls) P.dst.cls[o] = P.src.cls[s];
}

template <bool PIECES>
__global__ __launch_bounds__(PLANE_REDUCE_LANES) void dg_plane_nearest(PlaneReduceParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t cols[PLANE_REDUCE_SPAN];  // per source column of the run: its key over the band's rows
    const uint32_t tid = threadIdx.x, oy = blockIdx.y, f = blockIdx.z;
    uint32_t y0;
    const uint32_t ny = reduce_box(oy, P.fy, P.H, y0);
    const uint32_t ox0 = blockIdx.x * P.px_per_wg;
    const uint32_t np = min(P.px_per_wg, P.oW - ox0);                          // output pixels of this run
    const uint32_t c0 = P.fx * ox0;                                            // its source columns: [c0, c1)
    const uint32_t c1 = min(P.W, c0 + P.fx * np);
    const int16_t *const rows = P.src.distance + (size_t)f * P.src_px + (size_t)y0 * P.W;
    const uint32_t off0 = plane_band_keys<PIECES>(cols, rows, P.W, ny, c0, c1, tid);
    __syncthreads();
    for (uint32_t p = tid; p < np; p += PLANE_REDUCE_LANES) {
        uint32_t x0;
        const uint32_t nx = reduce_box(ox0 + p, P.fx, P.W, x0);
        const uint32_t *const e = cols + off0 + P.fx * p;
        uint32_t best = PLANE_KEY_NONE;
        for (uint32_t rx = 0; rx < nx; rx++) best = min(best, plane_box_key(e[rx], rx));
        plane_take<true>(P, f, ox0 + p, oy, x0 + plane_key_rx(best), y0 + plane_key_ry(best), plane_key_distance(best));
    }
}

__global__ __launch_bounds__(PLANE_REDUCE_LANES) void dg_plane_point(PlaneReduceParams P) {
    const uint32_t ox = blockIdx.x * PLANE_REDUCE_LANES + threadIdx.x, oy = blockIdx.y;
    if (ox >= P.oW) return;
    plane_take<false>(P, blockIdx.z, ox, oy, plane_point(ox, P.fx, P.W), plane_point(oy, P.fy, P.H), 0);
}

}  // namespace

hipError_t launch_plane_reduce(const PlaneReduceSrc &src, int W, int H, int n_frames, const dg_plane_reduce_desc &d, const PlaneReduceDst &dst,
                               hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    const bool nearest = d.rule == DG_PLANE_NEAREST;
    if (nearest && !src.distance) return hipErrorInvalidValue;
    PlaneReduceParams P{};
    P.W = (uint32_t)W; P.H = (uint32_t)H; P.fx = d.fx; P.fy = d.fy;
    P.oW = reduce_out_dim(P.W, d.fx); P.oH = reduce_out_dim(P.H, d.fy);
    P.px_per_wg = plane_reduce_px_per_wg(d.fx);
    P.src_px = (size_t)P.W * (size_t)P.H;
    P.dst_px = (size_t)P.oW * (size_t)P.oH;
    const bool pieces = P.W % 8u == 0u && reinterpret_cast<uintptr_t>(src.distance) % 16u == 0u;
    const uint32_t runs = nearest ? (P.oW + P.px_per_wg - 1u) / P.px_per_wg : (P.oW + PLANE_REDUCE_LANES - 1u) / PLANE_REDUCE_LANES;
    constexpr int kMaxZ = 65535;                               // frames per launch: the grid's z extent
    for (int f0 = 0; f0 < n_frames; f0 += kMaxZ) {
        const int nf = std::min(kMaxZ, n_frames - f0);
        const size_t s0 = (size_t)f0 * P.src_px, o0 = (size_t)f0 * P.dst_px;
        // (a source whose destination is missing is not read: the kernels test the destination)
        P.src = PlaneReduceSrc{src.distance ? src.distance + s0 : nullptr, src.kind ? src.kind + s0 : nullptr, src.id ? src.id + s0 : nullptr,
                               src.cls ? src.cls + s0 : nullptr};
        P.dst = PlaneReduceDst{dst.distance ? dst.distance + o0 : nullptr, dst.kind ? dst.kind + o0 : nullptr, dst.id ? dst.id + o0 : nullptr,
                               dst.cls ? dst.cls + o0 : nullptr};
        const dim3 grid(runs, P.oH, (unsigned)nf);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == n_frames ? stop : nullptr;
        if (!nearest) hipExtLaunchKernelGGL(dg_plane_point, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else if (pieces) hipExtLaunchKernelGGL(dg_plane_nearest<true>, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else hipExtLaunchKernelGGL(dg_plane_nearest<false>, grid, dim3(PLANE_REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
