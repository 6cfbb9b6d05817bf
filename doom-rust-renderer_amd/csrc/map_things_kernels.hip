// map_things_kernels.hip — map-object markers on the player-centred and floor-textured map frames.  The rules are
// map_things_core.h's; the band decomposition, the owner tile and the phases of the two plain kernels are ego_tile_phases.h's and
// floor_map_tile_phases.h's, taken as they stand.
//
// dg_ego_thing_tiles     dg_ego_tiles (ego_kernels.hip) with the things phase (ego_tile_things.h) behind its linedefs and arrow: one
//                        workgroup of 256 lanes per (frame, band), the same owner tile, list and counters in LDS and nothing else.  The
//                        resolve phase looks a marker edge's colour up in the marker table; every other word is dg_ego_tiles'.
// dg_floor_thing_tiles   dg_floor_map_tiles (floor_map_kernels.hip) likewise: the things phase runs before the floor phase, which fills
//                        only the pixels whose word is still 0 — a marker pixel keeps the marker's colour, like a line pixel.
// Every tile index, item and table index is bounds-checked.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "ego_tile_phases.h"
#include "ego_tile_things.h"
#include "floor_map_tile_phases.h"
#include "map_things_kernels.hpp"

namespace dg {

namespace {

constexpr int kThreads = kEgoThreads;
constexpr int kMaxY = kEgoMaxY;

template <uint32_t TILE, int PX>
__global__ void __launch_bounds__(kThreads) dg_ego_thing_tiles(EgoParams p, ThingParams t) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[TILE];
    __shared__ MapSeg list[EGO_CHUNK];
    __shared__ uint32_t n_list[2];
    const uint32_t f = blockIdx.y;
    EgoBand b;
    if (!ego_band<TILE>(p.W, p.H, b)) return;
    const EgoView v = p.views[f];
    const bool rotate = p.rotate != 0u;
    ego_tile_lines(tile, list, n_list, p.lines, p.words, p.n_lines, p.masks ? p.masks + (size_t)f * p.mask_words : nullptr,
                   p.arrow ? p.arrow + (size_t)3u * f : nullptr, v, p.scale, rotate, p.W, p.H, b);
    ego_tile_things(tile, list, n_list, t, f, v, p.scale, rotate, p.W, p.H, b);
    const ThingMarker *const markers = t.markers;
    const uint32_t n_things = t.n_things;
    ego_tile_store<PX>(tile, ego_band_out(p.fb, f, p.W, p.H, b), b.px,
                       [markers, n_things](uint32_t w) { return thing_is_value(w) ? thing_value_rgb(w, markers, n_things) : ego_value_rgb(w); });
}

template <uint32_t TILE, int PX>
__global__ void __launch_bounds__(kThreads) dg_floor_thing_tiles(FloorMapParams p, ThingParams t) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[TILE];
    __shared__ MapSeg list[EGO_CHUNK];
    __shared__ uint32_t n_list[2];
    const EgoParams &E = p.E;
    const uint32_t tid = threadIdx.x, f = blockIdx.y;
    const int32_t W = E.W, H = E.H;
    EgoBand b;
    if (!ego_band<TILE>(W, H, b)) return;
    const EgoView v = E.views[f];
    const bool rotate = E.rotate != 0u;
    ego_tile_lines(tile, list, n_list, E.lines, E.words, E.n_lines, E.masks ? E.masks + (size_t)f * E.mask_words : nullptr,
                   E.arrow ? E.arrow + (size_t)3u * f : nullptr, v, E.scale, rotate, W, H, b);
    ego_tile_things(tile, list, n_list, t, f, v, E.scale, rotate, W, H, b);
    const FloorCell *const row = p.cells + (size_t)f * p.T.n_sectors;
    const uint32_t *const seen = p.seen ? p.seen + (size_t)f * p.seen_words : nullptr;
    for (uint32_t j0 = 0; j0 < b.px; j0 += kThreads) {    // dg_floor_map_tiles' floor phase (the same trips for every lane: floor_lane's waves stay whole)
        const uint32_t j = j0 + tid;
        const bool want = j < b.px && tile[j] == 0u;
        float mx = 0.0f, my = 0.0f;
        if (want) {
            const uint32_t y = j / (uint32_t)W, x = j - y * (uint32_t)W;       // (an index, not the rule's arithmetic)
            floor_map_point((int32_t)x, b.row0 + (int32_t)y, W, H, v, p.inv, rotate, mx, my);
        }
        const uint32_t value = floor_lane(p.T, row, seen, want, mx, my);
        if (want) tile[j] = value;                        // j < px <= TILE
    }
    __syncthreads();
    const ThingMarker *const markers = t.markers;
    const uint32_t n_things = t.n_things;
    ego_tile_store<PX>(tile, ego_band_out(E.fb, f, W, H, b), b.px,
                       [markers, n_things](uint32_t w) { return thing_is_value(w) ? thing_value_rgb(w, markers, n_things) : floor_value_rgb(w); });
}

template <uint32_t TILE>
void launch_ego(int px_form, dim3 grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const EgoParams &q, const ThingParams &t) {
    if (px_form == 16) hipExtLaunchKernelGGL((dg_ego_thing_tiles<TILE, 16>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
    else if (px_form == 4) hipExtLaunchKernelGGL((dg_ego_thing_tiles<TILE, 4>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
    else hipExtLaunchKernelGGL((dg_ego_thing_tiles<TILE, 1>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
}

template <uint32_t TILE>
void launch_floor(int px_form, dim3 grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const FloorMapParams &q, const ThingParams &t) {
    if (px_form == 16) hipExtLaunchKernelGGL((dg_floor_thing_tiles<TILE, 16>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
    else if (px_form == 4) hipExtLaunchKernelGGL((dg_floor_thing_tiles<TILE, 4>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
    else hipExtLaunchKernelGGL((dg_floor_thing_tiles<TILE, 1>), grid, dim3(kThreads), 0, stream, ev0, ev1, 0, q, t);
}

bool ego_params_ok(const EgoParams &E) {
    if (E.W < 1 || E.H < 1 || E.W > (int32_t)EGO_WIDE_TILE_PX || E.H > 16384 || E.n_lines > EGO_MAX_LINES || !E.views || !E.fb) return false;
    if (E.n_lines > 0u && (!E.lines || !E.words)) return false;
    return !(E.masks && (size_t)E.mask_words * 32u < E.n_lines);
}

bool thing_params_ok(const ThingParams &t) {
    if (t.n_things == 0u) return true;
    if (t.n_things > THING_MAX || !t.markers || !t.places || !t.shown || !t.entries || !t.first) return false;
    return (size_t)t.shown_words * 32u >= t.n_things;
}

// The parameters of frames [f0, ..) of a launch: every per-frame pointer moved on.  (first[] holds places in the whole entry table.)
EgoParams ego_from(const EgoParams &p, int f0, int nf) {
    EgoParams q = p;
    q.views = p.views + f0;
    q.arrow = p.arrow ? p.arrow + (size_t)3 * f0 : nullptr;
    q.masks = p.masks ? p.masks + (size_t)f0 * p.mask_words : nullptr;
    q.fb = p.fb + (size_t)f0 * 3u * (size_t)p.W * (size_t)p.H;
    q.n_frames = nf;
    return q;
}
ThingParams things_from(const ThingParams &t, int f0) {
    ThingParams q = t;
    if (t.n_things) { q.shown = t.shown + (size_t)f0 * t.shown_words; q.first = t.first + f0; }
    return q;
}

}  // namespace

hipError_t launch_ego_thing_tiles(const EgoParams &p, const ThingParams &t, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (p.n_frames <= 0) return hipSuccess;
    if (!ego_params_ok(p) || !thing_params_ok(t)) return hipErrorInvalidValue;
    const uint32_t W = (uint32_t)p.W, H = (uint32_t)p.H, bands = ego_bands(W, H);
    const int px_form = (int)ego_store_px(W, H, (uint64_t)reinterpret_cast<uintptr_t>(p.fb));
    for (int f0 = 0; f0 < p.n_frames; f0 += kMaxY) {       // more frames than the grid's y extent take several launches
        const int nf = std::min(kMaxY, p.n_frames - f0);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == p.n_frames ? stop : nullptr;
        const EgoParams q = ego_from(p, f0, nf);
        const ThingParams u = things_from(t, f0);
        const dim3 grid(bands, (unsigned)nf);
        if (W > EGO_TILE_PX) launch_ego<EGO_WIDE_TILE_PX>(px_form, grid, stream, ev0, ev1, q, u);
        else launch_ego<EGO_TILE_PX>(px_form, grid, stream, ev0, ev1, q, u);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_floor_thing_tiles(const FloorMapParams &p, const ThingParams &t, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    const EgoParams &E = p.E;
    const FloorTables &T = p.T;
    if (E.n_frames <= 0) return hipSuccess;
    if (!ego_params_ok(E) || !thing_params_ok(t)) return hipErrorInvalidValue;
    if (!p.cells || !T.palette || !T.leaves || T.n_leaves == 0u || T.n_sectors == 0u || (T.n_nodes && !T.nodes) || (T.n_segs && !T.segs) || (T.n_flats && !T.flats))
        return hipErrorInvalidValue;
    if (T.n_nodes > 0x7fffffffu || (p.seen && (size_t)p.seen_words * 32u < T.n_sectors)) return hipErrorInvalidValue;
    const uint32_t W = (uint32_t)E.W, H = (uint32_t)E.H, bands = ego_bands(W, H);
    const int px_form = (int)ego_store_px(W, H, (uint64_t)reinterpret_cast<uintptr_t>(E.fb));
    for (int f0 = 0; f0 < E.n_frames; f0 += kMaxY) {
        const int nf = std::min(kMaxY, E.n_frames - f0);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == E.n_frames ? stop : nullptr;
        FloorMapParams q = p;
        q.E = ego_from(E, f0, nf);
        q.cells = p.cells + (size_t)f0 * T.n_sectors;
        q.seen = p.seen ? p.seen + (size_t)f0 * p.seen_words : nullptr;
        const ThingParams u = things_from(t, f0);
        const dim3 grid(bands, (unsigned)nf);
        if (W > EGO_TILE_PX) launch_floor<EGO_WIDE_TILE_PX>(px_form, grid, stream, ev0, ev1, q, u);
        else launch_floor<EGO_TILE_PX>(px_form, grid, stream, ev0, ev1, q, u);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
