// map_kernels.hip — the 2-D map view (src/game.rs:491-499 with viewing_map): a layer of every drawn linedef, built once per uploaded
// scene, and per frame a copy of it with the player arrow on top.  Line steps come from map_core.h; the host clips every line to the
// frame (map_seg_make) before upload, and every store below is still bounds-checked.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "map_kernels.hpp"

namespace dg {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

// One lane per (line, clipped step): the later line wins a pixel (atomicMax of line + 1), as the reference's later draw_line overwrites.
__global__ void __launch_bounds__(kThreads) dg_map_layer_steps(const MapSeg *__restrict__ segs, const uint32_t *__restrict__ base, uint32_t n,
                                                               uint32_t total, uint32_t *__restrict__ owner, int W, int H) {
    for (uint32_t lane = blockIdx.x * kThreads + threadIdx.x; lane < total; lane += gridDim.x * kThreads) {
        uint32_t lo = 0, hi = n;                           // the line k with base[k] <= lane < base[k + 1]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (base[mid] <= lane) lo = mid; else hi = mid;
        }
        const MapSeg s = segs[lo];
        int32_t x, y;
        map_seg_point(s, (int64_t)s.first + (int64_t)(lane - base[lo]), x, y);
        if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) atomicMax(&owner[(size_t)y * (size_t)W + (size_t)x], lo + 1);
    }
}

__global__ void __launch_bounds__(kThreads) dg_map_layer_resolve(const MapSeg *__restrict__ segs, const uint32_t *__restrict__ owner,
                                                                 uint8_t *__restrict__ layer, uint32_t pixels) {
    for (uint32_t p = blockIdx.x * kThreads + threadIdx.x; p < pixels; p += gridDim.x * kThreads) {
        const uint32_t o = owner[p];
        const uint32_t rgb = o ? segs[o - 1].rgb : 0u;
        layer[3 * (size_t)p + 0] = (uint8_t)rgb;
        layer[3 * (size_t)p + 1] = (uint8_t)(rgb >> 8);
        layer[3 * (size_t)p + 2] = (uint8_t)(rgb >> 16);
    }
}

// frame blockIdx.y = layer.  T: the widest of 16 / 4 / 1 bytes that divides the frame size, so every frame starts aligned to it.
// Non-temporal stores: the frames are written once and not read back by the GPU; the layer (3 MB at 1280x800) stays in L2 / MALL.
template <typename T>
__global__ void __launch_bounds__(kThreads) dg_map_copy(const T *__restrict__ layer, T *__restrict__ fb, uint32_t n_elems) {
    T *dst = fb + (size_t)blockIdx.y * n_elems;
    for (uint32_t j = blockIdx.x * kThreads + threadIdx.x; j < n_elems; j += gridDim.x * kThreads)
        __builtin_nontemporal_store(layer[j], dst + j);
}

// The arrow: line blockIdx.x of frame blockIdx.y, its clipped steps over the block's lanes; every arrow pixel is (255, 255, 0).
__global__ void __launch_bounds__(kThreads) dg_map_arrow(const MapSeg *__restrict__ arrow, uint8_t *__restrict__ fb, int W, int H) {
    const MapSeg s = arrow[3 * blockIdx.y + blockIdx.x];
    uint8_t *frame = fb + (size_t)blockIdx.y * 3 * (size_t)W * (size_t)H;
    for (int32_t k = (int32_t)threadIdx.x; k < s.count; k += kThreads) {
        int32_t x, y;
        map_seg_point(s, (int64_t)s.first + k, x, y);
        if ((uint32_t)x >= (uint32_t)W || (uint32_t)y >= (uint32_t)H) continue;
        uint8_t *px = frame + 3 * ((size_t)y * (size_t)W + (size_t)x);
        px[0] = (uint8_t)s.rgb; px[1] = (uint8_t)(s.rgb >> 8); px[2] = (uint8_t)(s.rgb >> 16);
    }
}

unsigned grid_for(size_t items, size_t per_block_cap) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + kThreads - 1) / kThreads, per_block_cap));
}

}  // namespace

hipError_t launch_map_layer(const MapSeg *segs, const uint32_t *base, uint32_t n, uint32_t total, uint32_t *owner, uint8_t *layer,
                            int W, int H, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    const uint32_t pixels = (uint32_t)W * (uint32_t)H;
    hipExtLaunchKernelGGL(dg_map_layer_steps, dim3(grid_for(total, 65536)), dim3(kThreads), 0, stream, start, nullptr, 0,
                          segs, base, n, total, owner, W, H);
    hipExtLaunchKernelGGL(dg_map_layer_resolve, dim3(grid_for(pixels, 65536)), dim3(kThreads), 0, stream, nullptr, stop, 0,
                          segs, (const uint32_t *)owner, layer, pixels);
    return hipGetLastError();
}

hipError_t launch_map_frames(const uint8_t *layer, const MapSeg *arrow, int n_frames, uint8_t *fb, int W, int H, hipStream_t stream,
                             hipEvent_t start, hipEvent_t stop) {
    const size_t fsz = (size_t)3 * (size_t)W * (size_t)H;
    // ~8 elements per lane: enough blocks per frame to fill the chip at any batch size, few enough to keep the loop
    if (fsz % 16 == 0) {
        const uint32_t ne = (uint32_t)(fsz / 16);
        hipExtLaunchKernelGGL(dg_map_copy<u32x4>, dim3(grid_for((ne + 7) / 8, 4096), (unsigned)n_frames), dim3(kThreads), 0, stream, start, nullptr, 0,
                              reinterpret_cast<const u32x4 *>(layer), reinterpret_cast<u32x4 *>(fb), ne);
    } else if (fsz % 4 == 0) {
        const uint32_t ne = (uint32_t)(fsz / 4);
        hipExtLaunchKernelGGL(dg_map_copy<uint32_t>, dim3(grid_for((ne + 7) / 8, 4096), (unsigned)n_frames), dim3(kThreads), 0, stream, start, nullptr, 0,
                              reinterpret_cast<const uint32_t *>(layer), reinterpret_cast<uint32_t *>(fb), ne);
    } else {
        const uint32_t ne = (uint32_t)fsz;
        hipExtLaunchKernelGGL(dg_map_copy<uint8_t>, dim3(grid_for((ne + 7) / 8, 4096), (unsigned)n_frames), dim3(kThreads), 0, stream, start, nullptr, 0,
                              layer, fb, ne);
    }
    return launch_map_arrow(arrow, n_frames, fb, W, H, stream, nullptr, stop);
}

hipError_t launch_map_arrow(const MapSeg *arrow, int n_frames, uint8_t *fb, int W, int H, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    hipExtLaunchKernelGGL(dg_map_arrow, dim3(3, (unsigned)n_frames), dim3(kThreads), 0, stream, start, stop, 0, arrow, fb, W, H);
    return hipGetLastError();
}

}  // namespace dg
