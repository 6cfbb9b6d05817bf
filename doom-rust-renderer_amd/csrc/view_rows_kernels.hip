// view_rows_kernels.hip — the seg walk's per-view rows when a batch carries entries for them: map-object poses (dg_view_poses,
// DESIGN.md §8m), sector heights (dg_view_sectors, §8n) and sector flats (dg_view_surfaces, §8p), one mechanism (§8q).  A kind's fill
// kernel: one lane per (frame, item), numbered in one row-major index so that a map with few items still fills its wavefronts;
// consecutive lanes store consecutive elements.  Its scatter kernel: one lane per entry, one load of the entry and one store of an
// element — for the poses with the BSP descent in between, which reads a node (24 B, cached: every lane starts at the root) per level,
// ten to thirty levels.  Both bodies are view_rows_core.h's, the host's too.  No LDS, no scratch, no atomics: the entries are unique
// per (frame, item), and the scatter follows the fill in stream order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "view_rows_kernels.hpp"

namespace dg {

namespace {

template <class K> __device__ __forceinline__ void fill_lane(const ViewRowParams<K> &P) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= P.n_frames * P.n_items) return;
    view_row_fill(P, idx);
}
template <class K> __device__ __forceinline__ void scatter_lane(const ViewRowParams<K> &P) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= P.n_entries) return;
    view_row_scatter(P, e);
}

// The kernels by the names the profiles, the ISA tests and DESIGN.md know them by.
__global__ __launch_bounds__(256) void dg_mobj_pose_fill(PoseParams P) { fill_lane(P); }
__global__ __launch_bounds__(256) void dg_mobj_pose_place(PoseParams P) { scatter_lane(P); }
__global__ __launch_bounds__(256) void dg_sector_row_fill(SectorRowParams P) { fill_lane(P); }
__global__ __launch_bounds__(256) void dg_sector_row_scatter(SectorRowParams P) { scatter_lane(P); }
__global__ __launch_bounds__(256) void dg_flat_row_fill(FlatRowParams P) { fill_lane(P); }
__global__ __launch_bounds__(256) void dg_flat_row_scatter(FlatRowParams P) { scatter_lane(P); }

template <class K> struct RowKernels;
template <> struct RowKernels<PoseRows> { static constexpr auto fill = dg_mobj_pose_fill, scatter = dg_mobj_pose_place; };
template <> struct RowKernels<HeightRows> { static constexpr auto fill = dg_sector_row_fill, scatter = dg_sector_row_scatter; };
template <> struct RowKernels<FlatRows> { static constexpr auto fill = dg_flat_row_fill, scatter = dg_flat_row_scatter; };

}  // namespace

template <class K> hipError_t launch_view_rows(const ViewRowParams<K> &P, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (!P.scene_rows || !P.rows || (P.n_entries && !P.entries) || !K::ctx_ok(P.ctx)) return hipErrorInvalidValue;
    if (P.n_frames == 0 || P.n_items == 0) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)P.n_frames * P.n_items;
    if (total >= (1ull << 31) || P.n_entries > total) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL(RowKernels<K>::fill, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, stream, start, P.n_entries ? nullptr : stop, 0, P);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;   // each launch checked: a later success would hide it
    if (P.n_entries) hipExtLaunchKernelGGL(RowKernels<K>::scatter, dim3((P.n_entries + 255u) / 256u), dim3(256), 0, stream, nullptr, stop, 0, P);
    return hipGetLastError();
}
template hipError_t launch_view_rows<PoseRows>(const PoseParams &, hipStream_t, hipEvent_t, hipEvent_t);
template hipError_t launch_view_rows<HeightRows>(const SectorRowParams &, hipStream_t, hipEvent_t, hipEvent_t);
template hipError_t launch_view_rows<FlatRows>(const FlatRowParams &, hipStream_t, hipEvent_t, hipEvent_t);

}  // namespace dg
