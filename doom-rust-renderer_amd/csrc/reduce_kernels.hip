// reduce_kernels.hip — the box downscale of RGB24 frames (dg_reduce_device, dg_readback_reduced*): a streaming kernel of
// its own beside the render path.  It reads 3*W*H bytes per frame once and writes fx*fy times fewer (3x fewer again as gray).
//
// One workgroup = one band of fy source rows of one frame x a run of whole output pixels (reduce_px_per_wg).
//   1. (reduce_band.h) every lane adds its bytes of the band's rows in registers, as 16-bit sums per byte position (<= 16 x 255), and puts them in LDS;
//      dg_reduce<true>: one 16-byte piece per lane and row, the pieces of a row consecutive and 16-byte aligned (3 W % 16 == 0, aligned
//      base), so the run starts up to 15 bytes in front of its first pixel; dg_reduce<false> (any width, any base): the lanes of a wave
//      read 64 consecutive bytes per load, 16 loads per row;
//   2. after one barrier, one lane per output byte adds the fx column sums of its channel and divides (reduce_round: a multiply-high by
//      one of the four reciprocals the host worked out);
//   3. DG_REDUCE_GRAY8 keeps those bytes in LDS and, after a second barrier, one lane per output pixel writes the luma.
// No float arithmetic, plain loads and stores.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "reduce_band.h"
#include "reduce_kernels.hpp"

namespace dg {

namespace {

struct ReduceParams {
    const uint8_t *src;
    uint8_t *dst;
    size_t src_frame, dst_frame;   // bytes per source / reduced frame
    uint32_t W, H, fx, fy, gray, oW, oH;
    uint32_t row_bytes;            // 3 W
    uint32_t px_per_wg;
    uint32_t rcp[4];               // reduce_rcp of the box sizes: [2 * (short box at the bottom edge) + (short box at the right edge)]
};

template <bool PIECES>
__global__ __launch_bounds__(REDUCE_LANES) void dg_reduce(ReduceParams P) {
    __shared__ __attribute__((aligned(16))) uint16_t sums[REDUCE_SPAN];        // per byte position of the run: its sum over the band's rows
    __shared__ uint8_t rgb[(3u * reduce_px_per_wg(1u) + 15u) & ~15u];          // DG_REDUCE_GRAY8: the run's rounded bytes
    const uint32_t tid = threadIdx.x, oy = blockIdx.y;
    uint32_t y0;
    const uint32_t ny = reduce_box(oy, P.fy, P.H, y0);
    const uint32_t ox0 = blockIdx.x * P.px_per_wg;
    const uint32_t np = min(P.px_per_wg, P.oW - ox0);                          // output pixels of this run
    const uint32_t b0 = 3u * P.fx * ox0;                                       // its source bytes within a row: [b0, b1)
    const uint32_t b1 = min(P.row_bytes, b0 + 3u * P.fx * np);
    const uint8_t *const rows = P.src + (size_t)blockIdx.z * P.src_frame + (size_t)y0 * P.row_bytes;
    const uint32_t off0 = reduce_band_sums<PIECES>(sums, rows, P.row_bytes, ny, b0, b1, tid);
    __syncthreads();
    const uint32_t rcp_full = P.rcp[ny < P.fy ? 2 : 0], rcp_short = P.rcp[ny < P.fy ? 3 : 1];
    uint8_t *const out = P.dst + (size_t)blockIdx.z * P.dst_frame + ((size_t)oy * P.oW + ox0) * (P.gray ? 1u : 3u);
    for (uint32_t j = tid; j < 3u * np; j += REDUCE_LANES) {
        const uint32_t p = j / 3u, c = j - 3u * p;
        uint32_t x0;
        const uint32_t nx = reduce_box(ox0 + p, P.fx, P.W, x0);
        const uint16_t *const e = sums + off0 + 3u * P.fx * p + c;
        uint32_t s = 0;
        for (uint32_t k = 0; k < nx; k++) s += e[3u * k];
        const uint8_t v = (uint8_t)reduce_round(s, nx * ny, nx < P.fx ? rcp_short : rcp_full);
        if (P.gray) rgb[j] = v;
        else out[j] = v;
    }
    if (P.gray) {
        __syncthreads();
        for (uint32_t p = tid; p < np; p += REDUCE_LANES) out[p] = (uint8_t)reduce_luma(rgb[3u * p], rgb[3u * p + 1u], rgb[3u * p + 2u]);
    }
}

}  // namespace

hipError_t launch_reduce(const uint8_t *src, int W, int H, int n_frames, const dg_reduce_desc &d, uint8_t *dst, hipStream_t stream,
                         hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    ReduceParams P{};
    P.W = (uint32_t)W; P.H = (uint32_t)H; P.fx = d.fx; P.fy = d.fy; P.gray = d.format == DG_REDUCE_GRAY8 ? 1u : 0u;
    P.oW = reduce_out_dim(P.W, d.fx); P.oH = reduce_out_dim(P.H, d.fy);
    P.row_bytes = 3u * P.W;
    P.px_per_wg = reduce_px_per_wg(d.fx);
    P.src_frame = (size_t)P.row_bytes * (size_t)P.H;
    P.dst_frame = reduce_frame_bytes(P.W, P.H, d);
    uint32_t lo;
    const uint32_t nx_last = reduce_box(P.oW - 1u, d.fx, P.W, lo), ny_last = reduce_box(P.oH - 1u, d.fy, P.H, lo);
    P.rcp[0] = reduce_rcp(d.fx * d.fy); P.rcp[1] = reduce_rcp(nx_last * d.fy);
    P.rcp[2] = reduce_rcp(d.fx * ny_last); P.rcp[3] = reduce_rcp(nx_last * ny_last);
    const bool pieces = P.row_bytes % 16u == 0u && reinterpret_cast<uintptr_t>(src) % 16u == 0u;
    const uint32_t runs = (P.oW + P.px_per_wg - 1u) / P.px_per_wg;
    constexpr int kMaxZ = 65535;                               // frames per launch: the grid's z extent
    for (int f0 = 0; f0 < n_frames; f0 += kMaxZ) {
        const int nf = std::min(kMaxZ, n_frames - f0);
        P.src = src + (size_t)f0 * P.src_frame;
        P.dst = dst + (size_t)f0 * P.dst_frame;
        const dim3 grid(runs, P.oH, (unsigned)nf);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == n_frames ? stop : nullptr;
        if (pieces) hipExtLaunchKernelGGL(dg_reduce<true>, grid, dim3(REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        else hipExtLaunchKernelGGL(dg_reduce<false>, grid, dim3(REDUCE_LANES), 0, stream, ev0, ev1, 0, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
