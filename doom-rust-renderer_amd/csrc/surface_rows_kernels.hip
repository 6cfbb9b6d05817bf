// surface_rows_kernels.hip — the seg walk's per-view sector flat rows when a batch carries surface entries (dg_view_surfaces,
// DESIGN.md §8p).  dg_flat_row_fill: one lane per (frame, sector), numbered in one row-major index so that a map with few sectors
// still fills its wavefronts; consecutive lanes store consecutive 8-byte elements.  dg_flat_row_scatter: one lane per entry, one
// 16-byte load and one 8-byte store.  Both bodies are surface_rows_core.h's, the host's too.  No LDS, no scratch, no atomics: the
// entries are unique per (frame, sector), and the scatter follows the fill in stream order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "surface_rows_kernels.hpp"

namespace dg {

namespace {

__global__ __launch_bounds__(256) void dg_flat_row_fill(FlatRowParams P) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= P.n_frames * P.n_sectors) return;
    flat_row_fill(P, idx);
}

__global__ __launch_bounds__(256) void dg_flat_row_scatter(FlatRowParams P) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= P.n_entries) return;
    flat_row_scatter(P, e);
}

}  // namespace

hipError_t launch_flat_rows(const FlatRowParams &P, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (!P.scene_rows || !P.rows || (P.n_entries && !P.entries)) return hipErrorInvalidValue;
    if (P.n_frames == 0 || P.n_sectors == 0) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)P.n_frames * P.n_sectors;
    if (total >= (1ull << 31) || P.n_entries > total) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(dg_flat_row_fill, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, stream, start, P.n_entries ? nullptr : stop, 0, P);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (P.n_entries) hipExtLaunchKernelGGL(dg_flat_row_scatter, dim3((P.n_entries + 255u) / 256u), dim3(256), 0, stream, nullptr, stop, 0, P);
    return hipGetLastError();
}

}  // namespace dg
