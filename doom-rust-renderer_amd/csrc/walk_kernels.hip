// walk_kernels.hip — the floor heights of recorded walks (dg_ctx_locate_walks).  The probes of all walks of a call are
// concatenated; dg_walk_locate descends the BSP once per probe (walk_core.h, the host path's body), and "keep the last lookup that hit
// a sector" is an inclusive max-scan of valid ? index : 0 over all probes.  A walk's first probe is always valid (0.0 when it misses),
// so the carry never crosses a walk boundary and the scan needs no segment logic.
// The scan is reduce, scan of the block maxima, apply — three launches, wave64 scans inside a workgroup, and no workgroup ever waits
// on another.  Plain loads and stores; the descent's node reads are a few cached words per level.
#include <hip/hip_runtime.h>

#include "walk_kernels.hpp"

namespace dg {

namespace {

constexpr uint32_t WALK_LANES = 256;
constexpr uint32_t WALK_PER_LANE = WALK_SCAN_BLOCK / WALK_LANES;

__device__ __forceinline__ uint32_t walk_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Inclusive max-scan over the 64 lanes of a wavefront.
__device__ __forceinline__ uint32_t walk_wave_scan(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v = walk_max(v, o);
    }
    return v;
}

// Over the 256 lanes of a workgroup: `incl` becomes the inclusive max-scan of v, the return value is the maximum of all 256.
// wv: 4 words of shared memory, free again after the call (it ends in a barrier).
__device__ __forceinline__ uint32_t walk_group_scan(uint32_t v, uint32_t *wv, uint32_t &incl, uint32_t &excl) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t in_wave = walk_wave_scan(v, lane);
    const uint32_t before = __shfl_up(in_wave, 1, 64);
    if (lane == 63u) wv[wave] = in_wave;
    __syncthreads();
    uint32_t pre = 0, all = 0;
    for (uint32_t w = 0; w < WALK_LANES / 64u; w++) {
        const uint32_t t = wv[w];
        if (w < wave) pre = walk_max(pre, t);
        all = walk_max(all, t);
    }
    excl = lane ? walk_max(pre, before) : pre;
    incl = walk_max(pre, in_wave);
    __syncthreads();
    return all;
}

__global__ __launch_bounds__(256) void dg_walk_locate(WalkParams P) {
    const uint32_t i = blockIdx.x * WALK_LANES + threadIdx.x;
    if (i >= P.n_probes) return;
    float v = 0.0f;
    const bool hit = walk_floor_at(P.nodes, P.root, P.leaves, P.x[i], P.y[i], v);
    P.value[i] = v;
    P.last[i] = (hit || P.first[i]) ? i : 0u;
}

__global__ __launch_bounds__(256) void dg_walk_block_max(WalkParams P) {
    __shared__ uint32_t wv[WALK_LANES / 64u];
    const uint32_t base = blockIdx.x * WALK_SCAN_BLOCK;
    uint32_t m = 0;
    for (uint32_t k = 0; k < WALK_PER_LANE; k++) {
        const uint32_t i = base + k * WALK_LANES + threadIdx.x;
        if (i < P.n_probes) m = walk_max(m, P.last[i]);
    }
    uint32_t incl, excl;
    const uint32_t all = walk_group_scan(m, wv, incl, excl);
    if (threadIdx.x == 0) P.sums[blockIdx.x] = all;
}

// One workgroup: sums[b] becomes the maximum of all blocks before b (0 for the first).
__global__ __launch_bounds__(256) void dg_walk_scan_sums(WalkParams P) {
    __shared__ uint32_t wv[WALK_LANES / 64u];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < P.n_blocks; base += WALK_LANES) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < P.n_blocks ? P.sums[b] : 0u;
        uint32_t incl, excl;
        const uint32_t all = walk_group_scan(v, wv, incl, excl);
        if (b < P.n_blocks) P.sums[b] = walk_max(carry, excl);
        carry = walk_max(carry, all);
    }
}

__global__ __launch_bounds__(256) void dg_walk_scan_apply(WalkParams P) {
    __shared__ uint32_t wv[WALK_LANES / 64u];
    const uint32_t first = blockIdx.x * WALK_SCAN_BLOCK + threadIdx.x * WALK_PER_LANE;
    uint32_t a[WALK_PER_LANE];
    uint32_t m = 0;
    for (uint32_t k = 0; k < WALK_PER_LANE; k++) {
        const uint32_t i = first + k;
        m = walk_max(m, i < P.n_probes ? P.last[i] : 0u);
        a[k] = m;
    }
    uint32_t incl, excl;
    (void)walk_group_scan(m, wv, incl, excl);
    const uint32_t pre = walk_max(P.sums[blockIdx.x], excl);
    for (uint32_t k = 0; k < WALK_PER_LANE; k++) {
        const uint32_t i = first + k;
        if (i < P.n_probes) P.last[i] = walk_max(pre, a[k]);
    }
}

__global__ __launch_bounds__(256) void dg_walk_gather(WalkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * WALK_LANES + threadIdx.x;
    if (e >= P.n_entries) return;
    P.floors[e] = P.value[P.last[P.end_of_tic[e]]];
}

}  // namespace

hipError_t launch_walk_locate(const WalkParams &P, hipStream_t stream) {
    if (!P.nodes || !P.leaves || !P.x || !P.y || !P.first || !P.end_of_tic || !P.value || !P.last || !P.sums || !P.floors) return hipErrorInvalidValue;
    if (P.n_probes == 0 || P.n_probes > WALK_MAX_PROBES || P.root < 0) return hipErrorInvalidValue;
    if (P.n_blocks != (P.n_probes + WALK_SCAN_BLOCK - 1u) / WALK_SCAN_BLOCK) return hipErrorInvalidValue;
    const uint64_t gather_groups = (P.n_entries + WALK_LANES - 1u) / WALK_LANES;
    if (gather_groups >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dg_walk_locate, dim3((P.n_probes + WALK_LANES - 1u) / WALK_LANES), dim3(WALK_LANES), 0, stream, P);
    hipLaunchKernelGGL(dg_walk_block_max, dim3(P.n_blocks), dim3(WALK_LANES), 0, stream, P);
    hipLaunchKernelGGL(dg_walk_scan_sums, dim3(1), dim3(WALK_LANES), 0, stream, P);
    hipLaunchKernelGGL(dg_walk_scan_apply, dim3(P.n_blocks), dim3(WALK_LANES), 0, stream, P);
    if (gather_groups) hipLaunchKernelGGL(dg_walk_gather, dim3((unsigned)gather_groups), dim3(WALK_LANES), 0, stream, P);
    return hipGetLastError();
}

}  // namespace dg
