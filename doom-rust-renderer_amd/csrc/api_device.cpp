// api_device.cpp — the entry points of the C-ABI (include/doomgpu.h) that take a dg_ctx and are no part of a slot's lifecycle: each
// runs on a stream of the ctx's own, created by its first use, and returns when its work is done.  The box downscale of frames in device
// memory (dg_reduce_device), the reduced depth and label planes (dg_reduce_planes_device), the observation tensors
// (dg_observe_device), the screen pictures over colour frames (dg_overlay_device, dg_slot_overlay — which draws on a slot's frames once
// they are final), the linedefs seen in label planes (dg_seen_lines_device, dg_slot_seen_lines — the one call here that reads a slot, once its submission is final), the
// line-of-sight queries (dg_sight_device, dg_sight_mobjs_device), the floor heights of recorded walks (dg_ctx_locate_walks), and the getters of their kernels' times.  The readbacks of a slot's frames and planes:
// api_readback.cpp.  Slot, dg_ctx and the slot helpers: context.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "context.hpp"
#include "explored_kernels.hpp"
#include "observe_kernels.hpp"
#include "overlay_kernels.hpp"
#include "plane_reduce_kernels.hpp"
#include "reduce_kernels.hpp"
#include "sight_host.hpp"
#include "sight_kernels.hpp"
#include "walk.hpp"
#include "walk_kernels.hpp"

using namespace dg;

// A side stream of the ctx (xstream, wstream): created by the first call that uses it, non-blocking.
static hipError_t side_stream(Stream &s) { return s ? hipSuccess : stream_create(s); }

// The tail of every call here: whatever was queued on `stream` has run when this returns.  e: what the queueing returned; the first
// error of the two is reported under the call's name.
static int finish(hipStream_t stream, hipError_t e, const char *name) {
    const hipError_t es = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_err(DG_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
    return DG_OK;
}

extern "C" {

int dg_reduce_device(dg_ctx *c, const void *src, int width, int height, int n_frames, const dg_reduce_desc *desc, void *dst) {
    if (!c || !src || !dst) return set_err(DG_ERR_INVALID, "null argument");
    const int rc = check_reduce_desc(desc);
    if (rc) return rc;
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || n_frames < 0) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384], n_frames >= 0");
    if (n_frames == 0) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(side_stream(c->xstream));
    HIP_TRY(c->reduce.begin());
    const hipStream_t xs = c->xstream.get();
    const hipError_t e = launch_reduce(static_cast<const uint8_t *>(src), width, height, n_frames, *desc, static_cast<uint8_t *>(dst), xs, c->reduce.t0.get(), c->reduce.t1.get());
    if (const int bad = finish(xs, e, "dg_reduce_device")) return bad;
    c->reduce.end();
    return DG_OK;
}

int dg_ctx_reduce_kernel_ms(dg_ctx *c, float *ms) {
    if (!c || !ms) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->reduce.measured) return set_err(DG_ERR_INVALID, "no dg_reduce_device call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(c->reduce.elapsed(ms));
    return DG_OK;
}

int dg_reduce_planes_device(dg_ctx *c, int width, int height, int n_frames, const dg_plane_reduce_desc *desc,
                            const int16_t *distance, const uint8_t *kind, const uint16_t *id, const uint8_t *cls,
                            int16_t *o_distance, uint8_t *o_kind, uint16_t *o_id, uint8_t *o_cls) {
    if (!c) return set_err(DG_ERR_INVALID, "null argument");
    int rc = check_plane_reduce(width, height, n_frames, desc);
    if (!rc) rc = check_plane_pairs(*desc, distance, kind, id, cls, o_distance, o_kind, o_id, o_cls);
    if (rc) return rc;
    for (const void *p : {(const void *)distance, (const void *)id, (const void *)o_distance, (const void *)o_id})
        if (reinterpret_cast<uintptr_t>(p) % 2u) return set_err(DG_ERR_INVALID, "dg_reduce_planes_device: a 16-bit plane must be 2-byte aligned");
    if (n_frames == 0 || !(distance || kind || id || cls)) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(side_stream(c->xstream));
    HIP_TRY(c->plane_reduce.begin());
    const hipStream_t xs = c->xstream.get();
    const hipError_t e = launch_plane_reduce(PlaneReduceSrc{distance, kind, id, cls}, width, height, n_frames, *desc, PlaneReduceDst{o_distance, o_kind, o_id, o_cls},
                                             xs, c->plane_reduce.t0.get(), c->plane_reduce.t1.get());
    if ((rc = finish(xs, e, "dg_reduce_planes_device"))) return rc;
    c->plane_reduce.end();
    return DG_OK;
}

int dg_ctx_plane_reduce_kernel_ms(dg_ctx *c, float *ms) {
    if (!c || !ms) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->plane_reduce.measured) return set_err(DG_ERR_INVALID, "no dg_reduce_planes_device call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(c->plane_reduce.elapsed(ms));
    return DG_OK;
}

int dg_observe_device(dg_ctx *c, const void *src, int width, int height, int n_frames, const dg_obs_desc *desc, void *dst, const int64_t strides[4]) {
    if (!c) return set_err(DG_ERR_INVALID, "null argument");
    int rc = check_observe_call(src, width, height, n_frames, desc, dst, strides);
    if (rc) return rc;
    if (n_frames == 0) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(side_stream(c->xstream));
    HIP_TRY(c->observe.begin());
    const hipStream_t xs = c->xstream.get();
    const hipError_t e = launch_observe(src, width, height, n_frames, *desc, dst, strides, xs, c->observe.t0.get(), c->observe.t1.get());
    if ((rc = finish(xs, e, "dg_observe_device"))) return rc;
    c->observe.end();
    return DG_OK;
}

int dg_ctx_observe_kernel_ms(dg_ctx *c, float *ms) {
    if (!c || !ms) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->observe.measured) return set_err(DG_ERR_INVALID, "no dg_observe_device call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(c->observe.elapsed(ms));
    return DG_OK;
}

// dg_overlay_device and dg_slot_overlay once they know the frames: the plan's records into the ctx's scratch (items, then the rectangle
// records on a 256-byte boundary), the kernel, and the wait.  A plan without rectangles launches nothing.
static int overlay_frames(dg_ctx *c, uint8_t *frames, int width, int height, const OvlPlan &plan, const char *name) {
    if (plan.rects.empty()) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(side_stream(c->xstream));
    const size_t item_bytes = plan.items.size() * sizeof(OvlItem), rects_at = (item_bytes + 255) & ~(size_t)255;
    const size_t rect_bytes = plan.rects.size() * sizeof(OvlRect), total = rects_at + rect_bytes;
    if (total > c->overlay_cap) {
        c->overlay_cap = 0;
        const size_t cap = (total + 65535) & ~(size_t)65535;
        HIP_TRY(hip_alloc(c->d_overlay, cap));
        c->overlay_cap = cap;
    }
    HIP_TRY(c->overlay.begin());
    const hipStream_t xs = c->xstream.get();
    uint8_t *const d = c->d_overlay.get();
    hipError_t e = hipMemcpyAsync(d, plan.items.data(), item_bytes, hipMemcpyHostToDevice, xs);
    if (e == hipSuccess) e = hipMemcpyAsync(d + rects_at, plan.rects.data(), rect_bytes, hipMemcpyHostToDevice, xs);
    if (e == hipSuccess)
        e = launch_overlay(frames, width, height, reinterpret_cast<const OvlRect *>(d + rects_at), (uint32_t)plan.rects.size(), plan.max_tiles,
                           reinterpret_cast<const OvlItem *>(d), c->d_palette.get(), c->d_texel_idx.get(), c->d_texel_opq.get(), xs, c->overlay.t0.get(), c->overlay.t1.get());
    if (const int bad = finish(xs, e, name)) return bad;             // before the plan goes, whatever was queued has run
    c->overlay.end();
    return DG_OK;
}

int dg_overlay_device(dg_ctx *c, void *frames, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first) {
    if (!c || !frames) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    OvlPlan plan;
    if (const int rc = overlay_checked_plan(c->pictures, width, height, n_frames, items, first, plan)) return rc;
    return overlay_frames(c, static_cast<uint8_t *>(frames), width, height, plan, "dg_overlay_device");
}

int dg_slot_overlay(dg_ctx *c, int slot, int first_frame, int count, const dg_screen_picture *items, const uint32_t *first) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    Slot &s = c->slots[(size_t)slot];
    if ((rc = refuse_no_colour(s, "dg_slot_overlay"))) return rc;
    if (first_frame < 0 || count < 0 || first_frame > s.n_frames || count > s.n_frames - first_frame) return set_err(DG_ERR_INVALID, "bad frame range");
    if (s.phase == Slot::Phase::Prepared) return set_err(DG_ERR_INVALID, "dg_slot_overlay: the slot's views are prepared and have not run (dg_replay_slot)");
    if (s.copy_pending) return set_err(DG_ERR_INVALID, "dg_slot_overlay: an asynchronous readback of the slot is pending (dg_wait completes it)");
    OvlPlan plan;
    if ((rc = overlay_checked_plan(c->pictures, c->cfg.width, c->cfg.height, count, items, first, plan))) return rc;
    if (plan.rects.empty()) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = make_final(c, s, Copy::Leave))) return rc;
    const size_t W = (size_t)c->cfg.width, H = (size_t)c->cfg.height;
    uint8_t *const frames = s.d_fb.get() + s.layout(W, H).colour + (size_t)first_frame * 3u * W * H;
    return overlay_frames(c, frames, c->cfg.width, c->cfg.height, plan, "dg_slot_overlay");
}

int dg_ctx_overlay_kernel_ms(dg_ctx *c, float *ms) {
    if (!c || !ms) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->overlay.measured) return set_err(DG_ERR_INVALID, "no dg_overlay_device or dg_slot_overlay call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(c->overlay.elapsed(ms));
    return DG_OK;
}

// What dg_seen_lines_device and dg_slot_seen_lines need of the ctx: the no-slot stream, the uploaded scene's seg -> linedef table, and
// their two intervals, unmeasured until the call has run.
static int ensure_seen(dg_ctx *c) {
    HIP_TRY(side_stream(c->xstream));
    if (!c->per_scene.seg_line) {
        const Scene &sc = *c->scene;
        std::vector<uint32_t> table(std::max<size_t>(sc.segs.size(), 4), 0u);
        for (size_t k = 0; k < sc.segs.size(); k++) table[k] = (uint32_t)sc.segs[k].linedef;
        DevPtr<uint32_t> d_table;
        HIP_TRY(hip_alloc(d_table, table.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(d_table.get(), table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->per_scene.seg_line = std::move(d_table);
    }
    HIP_TRY(c->seen.begin());
    HIP_TRY(c->seen_acc.begin());
    return DG_OK;
}

int dg_seen_lines_device(dg_ctx *c, int width, int height, int n, const uint16_t *id, const uint8_t *cls, uint32_t *seen) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    int rc = check_seen_lines(c->scene, width, height, n, id, cls, seen);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(id) % 2u || reinterpret_cast<uintptr_t>(seen) % 4u)
        return set_err(DG_ERR_INVALID, "dg_seen_lines_device: the id plane must be 2-byte aligned, the seen rows 4-byte aligned");
    const uint32_t words = seen_words((uint32_t)c->scene->linedefs.size());
    if (n == 0 || words == 0) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = ensure_seen(c))) return rc;
    const hipStream_t xs = c->xstream.get();
    hipError_t e = hipMemsetAsync(seen, 0, (size_t)n * words * sizeof(uint32_t), xs);
    if (e == hipSuccess)
        e = launch_seen_lines(id, cls, width, height, n, c->per_scene.seg_line.get(), (uint32_t)c->scene->segs.size(), seen, words, xs, c->seen.t0.get(), c->seen.t1.get());
    if ((rc = finish(xs, e, "dg_seen_lines_device"))) return rc;
    c->seen.end();                                        // (no accumulate kernel ran: that interval stays unmeasured)
    return DG_OK;
}

int dg_slot_seen_lines(dg_ctx *c, int slot, int first, int count, int run_len, const uint32_t *carry_in, uint32_t *upto, uint32_t *total,
                       uint32_t *fresh, uint32_t *carry_out) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (!s.holds(BUNDLE_LABELS))
        return set_err(DG_ERR_INVALID, s.holds_bundle() ? "dg_slot_seen_lines: the slot's bundle has no label part (DG_BUNDLE_LABELS)"
                                                        : "dg_slot_seen_lines: the slot's last submission is not a label submission");
    if (first < 0 || count < 0 || first + count > s.n_frames) return set_err(DG_ERR_INVALID, "bad frame range");
    const size_t words = seen_words((uint32_t)c->scene->linedefs.size());
    if ((rc = check_seen_runs((int)std::max<size_t>(words, 1), count, run_len))) return rc;
    if (count == 0 || words == 0) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = make_final(c, s, Copy::Leave))) return rc;
    if ((rc = ensure_seen(c))) return rc;
    // scratch rows: seen | upto | carry_in | carry_out (max_batch rows each), then total | fresh (max_batch entries each)
    const size_t rows = (size_t)c->cfg.max_batch, block = rows * words;
    if (!c->per_scene.seen_scratch) HIP_TRY(hip_alloc(c->per_scene.seen_scratch, (4 * block + 2 * rows) * sizeof(uint32_t)));
    uint32_t *const d_seen = c->per_scene.seen_scratch.get(), *const d_upto = d_seen + block, *const d_cin = d_upto + block, *const d_cout = d_cin + block;
    uint32_t *const d_total = d_cout + block, *const d_fresh = d_total + rows;
    const size_t W = (size_t)c->cfg.width, H = (size_t)c->cfg.height, runs = (size_t)(count / run_len);
    const BundleLayout L = s.layout(W, H);
    const uint16_t *const id = reinterpret_cast<const uint16_t *>(s.d_fb.get() + L.id) + (size_t)first * W * H;
    const uint8_t *const cls = s.d_fb.get() + L.cls + (size_t)first * W * H;
    const hipStream_t xs = c->xstream.get();
    hipError_t e = hipMemsetAsync(d_seen, 0, (size_t)count * words * sizeof(uint32_t), xs);
    if (e == hipSuccess && carry_in) e = hipMemcpyAsync(d_cin, carry_in, runs * words * sizeof(uint32_t), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess)
        e = launch_seen_lines(id, cls, (int)W, (int)H, count, c->per_scene.seg_line.get(), (uint32_t)c->scene->segs.size(), d_seen, (uint32_t)words, xs, c->seen.t0.get(), c->seen.t1.get());
    if (e == hipSuccess)
        e = launch_seen_accumulate(d_seen, (uint32_t)words, count, run_len, carry_in ? d_cin : nullptr, d_upto, total ? d_total : nullptr,
                                   fresh ? d_fresh : nullptr, carry_out ? d_cout : nullptr, xs, c->seen_acc.t0.get(), c->seen_acc.t1.get());
    if (e == hipSuccess && upto) e = hipMemcpyAsync(upto, d_upto, (size_t)count * words * sizeof(uint32_t), hipMemcpyDeviceToHost, xs);
    if (e == hipSuccess && total) e = hipMemcpyAsync(total, d_total, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, xs);
    if (e == hipSuccess && fresh) e = hipMemcpyAsync(fresh, d_fresh, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, xs);
    if (e == hipSuccess && carry_out) e = hipMemcpyAsync(carry_out, d_cout, runs * words * sizeof(uint32_t), hipMemcpyDeviceToHost, xs);
    if ((rc = finish(xs, e, "dg_slot_seen_lines"))) return rc;      // before the caller's rows are read or reused, whatever was queued has run
    c->seen.end(); c->seen_acc.end();
    return DG_OK;
}

int dg_ctx_seen_kernel_ms(dg_ctx *c, float *lines_ms, float *accumulate_ms) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (!c->seen.measured) return set_err(DG_ERR_INVALID, "no dg_seen_lines_device or dg_slot_seen_lines call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (lines_ms) HIP_TRY(c->seen.elapsed(lines_ms));
    if (accumulate_ms) { *accumulate_ms = 0.0f; if (c->seen_acc.measured) HIP_TRY(c->seen_acc.elapsed(accumulate_ms)); }
    return DG_OK;
}

}  // extern "C"

// What dg_sight_device and dg_sight_mobjs_device need of the ctx before they queue anything: a scene the kernels' stacks hold (its BSP at
// most SIGHT_MAX_DEPTH deep, its children in 16 bits), the no-slot stream, and the scene's sight tables on the device.  Nothing is
// launched and no interval is touched when the scene is refused.
static int ensure_sight(dg_ctx *c) {
    const Scene &sc = *c->scene;
    dg_ctx::PerScene &ps = c->per_scene;
    if (!ps.sight_depth) ps.sight_depth = sight_scene_depth(sc);
    if (ps.sight_depth > SIGHT_MAX_DEPTH)
        return set_err(DG_ERR_CAPACITY, "the scene's BSP is " + std::to_string(ps.sight_depth) + " nodes deep: the device sight calls take " + std::to_string(SIGHT_MAX_DEPTH) +
                                            " at the most (dg_sight_host has no limit)");
    if (sc.walk_nodes.size() > 32768u || sc.subsectors.size() > 32768u) return set_err(DG_ERR_CAPACITY, "the device sight calls take 32 768 nodes and subsectors at the most");
    if (sc.subsectors.empty() || sc.sectors.empty()) return set_err(DG_ERR_INVALID, "sight queries: the scene has no subsectors");
    HIP_TRY(side_stream(c->xstream));
    if (!ps.sight_table) {
        SightHostTables H;
        sight_tables(sc, H);
        TablePack t;
        const size_t nodes = t.add(sc.walk_nodes), leaves = t.add(H.leaves), seg_line = t.add(H.seg_line), lines = t.add(H.lines);
        const size_t heights = t.add(sc.fs_heights), mobjs = t.add(sc.fs_mobjs), leaf_sector = t.add(sc.walk_leaf_sector);
        DevPtr<uint8_t> d_table;
        const hipError_t e = t.upload(d_table);
        if (e != hipSuccess) return set_err(DG_ERR_HIP, std::string("sight tables: ") + hipGetErrorString(e));
        ps.sight_T = SightTables{t.at<WalkNode>(nodes), (uint32_t)sc.walk_nodes.size(), t.at<FloorLeaf>(leaves), (uint32_t)H.leaves.size(), t.at<uint32_t>(seg_line),
                                 (uint32_t)H.seg_line.size(), t.at<SightLine>(lines), (uint32_t)H.lines.size(), t.at<FsHeights>(heights), (uint32_t)sc.sectors.size(), 1u};
        ps.sight_mobjs = t.at<FsMobj>(mobjs);
        ps.sight_leaf_sector = t.at<int32_t>(leaf_sector);
        ps.sight_table = std::move(d_table);
    }
    return DG_OK;
}

// A call's block in device memory: the parts a caller take()s lie on 256-byte boundaries.
static int sight_io(dg_ctx *c, size_t bytes) {
    dg_ctx::PerScene &ps = c->per_scene;
    if (bytes <= ps.sight_io_cap) return DG_OK;
    ps.sight_io_cap = 0;
    const size_t cap = (bytes + 65535) & ~(size_t)65535;
    HIP_TRY(hip_alloc(ps.sight_io, cap));
    ps.sight_io_cap = cap;
    return DG_OK;
}

// The rows of a call whose frames have entries, queued on xs after the entries' copies: the height rows into the ctx's sight_rows (T
// then reads them), the pose rows into its sight_poses (poses / pose_frames then name them).  d_he / d_pe: the entries in device
// memory.  The ctx's sight_rows interval spans the kernels launched here.
static hipError_t sight_queue_rows(dg_ctx *c, hipStream_t xs, int n_frames, const SectorEntry *d_he, size_t n_he, const PoseEntry *d_pe, size_t n_pe, SightTables &T,
                                   const FsMobj *&poses, uint32_t &pose_frames) {
    dg_ctx::PerScene &ps = c->per_scene;
    hipError_t e = hipSuccess;
    if (n_he) {
        const SectorRowParams P{T.rows, d_he, ps.sight_rows.get(), T.n_sectors, (uint32_t)n_frames, (uint32_t)n_he};
        e = launch_view_rows<HeightRows>(P, xs, c->sight_rows.t0.get(), n_pe ? nullptr : c->sight_rows.t1.get());
        T.rows = ps.sight_rows.get();
        T.row_frames = (uint32_t)n_frames;
    }
    if (e == hipSuccess && n_pe) {
        const PoseParams P{ps.sight_mobjs, d_pe, ps.sight_poses.get(), (uint32_t)c->scene->mobjs.size(), (uint32_t)n_frames, (uint32_t)n_pe,
                           PoseCtx{T.nodes, ps.sight_leaf_sector, (int32_t)T.n_nodes - 1}};
        e = launch_view_rows<PoseRows>(P, xs, n_he ? nullptr : c->sight_rows.t0.get(), c->sight_rows.t1.get());
        poses = ps.sight_poses.get();
        pose_frames = (uint32_t)n_frames;
    }
    return e;
}

extern "C" {

int dg_sight_device(dg_ctx *c, const dg_view_sectors *sectors, int n_frames, const dg_sight_query *q, int n, uint8_t *visible_out) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const Scene &sc = *c->scene;
    std::string err;
    int rc = sight_check_queries(&sc, n_frames, q, n, visible_out, err);
    if (rc) return set_err(rc, err);
    if (n_frames > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "n_frames exceeds max_batch");
    if (n == 0) return DG_OK;
    std::vector<SectorEntry> he;
    if ((rc = sight_sector_entries(sc, sectors, n_frames, c->arenas[0]->heights, he, err))) return set_err(rc, err);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = ensure_sight(c))) return rc;
    dg_ctx::PerScene &ps = c->per_scene;
    SlabCursor cur;
    const size_t at_he = cur.take(he.size() * sizeof(SectorEntry)), at_q = cur.take((size_t)n * sizeof(dg_sight_query)), at_out = cur.take((size_t)n);
    if ((rc = sight_io(c, cur.next))) return rc;
    if (!he.empty() && !ps.sight_rows) HIP_TRY(hip_alloc(ps.sight_rows, (size_t)c->cfg.max_batch * sc.sectors.size() * sizeof(FsHeights)));
    HIP_TRY(c->sight.begin());
    c->sight_rows.measured = false;
    if (!he.empty()) HIP_TRY(c->sight_rows.begin());
    const hipStream_t xs = c->xstream.get();
    uint8_t *const d = ps.sight_io.get();
    SightQueryParams P{ps.sight_T, reinterpret_cast<const dg_sight_query *>(d + at_q), d + at_out, (uint32_t)n};
    const FsMobj *no_poses = nullptr;
    uint32_t no_pose_frames = 1;
    hipError_t e = hipMemcpyAsync(d + at_q, q, (size_t)n * sizeof(dg_sight_query), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess && !he.empty()) e = hipMemcpyAsync(d + at_he, he.data(), he.size() * sizeof(SectorEntry), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess) e = sight_queue_rows(c, xs, n_frames, reinterpret_cast<const SectorEntry *>(d + at_he), he.size(), nullptr, 0, P.T, no_poses, no_pose_frames);
    if (e == hipSuccess) e = launch_sight_queries(P, xs, c->sight.t0.get(), c->sight.t1.get());
    if (e == hipSuccess) e = hipMemcpyAsync(visible_out, d + at_out, (size_t)n, hipMemcpyDeviceToHost, xs);
    if ((rc = finish(xs, e, "dg_sight_device"))) return rc;           // before the entries go and the caller reads, whatever was queued has run
    c->sight.end();
    if (!he.empty()) c->sight_rows.end();
    return DG_OK;
}

int dg_sight_mobjs_device(dg_ctx *c, const dg_view *views, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, float eye_height,
                          const float *mobj_height, uint32_t *visible_out) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const Scene &sc = *c->scene;
    std::string err;
    int rc = sight_check_mobjs(&sc, views, n, mobj_height, visible_out, err);
    if (rc) return set_err(rc, err);
    if (n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "n exceeds max_batch");
    if (n == 0) return DG_OK;
    std::vector<SectorEntry> he;
    std::vector<PoseEntry> pe;
    if ((rc = sight_sector_entries(sc, sectors, n, c->arenas[0]->heights, he, err))) return set_err(rc, err);
    if ((rc = sight_pose_entries(sc, poses, n, c->arenas[0]->poses, pe, err))) return set_err(rc, err);
    const size_t M = sc.mobjs.size(), words = sight_words(sc);
    if (M == 0) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = ensure_sight(c))) return rc;
    dg_ctx::PerScene &ps = c->per_scene;
    std::vector<SightView> sv;
    sight_views(views, n, eye_height, sv);
    SlabCursor cur;
    const size_t at_he = cur.take(he.size() * sizeof(SectorEntry)), at_pe = cur.take(pe.size() * sizeof(PoseEntry)), at_v = cur.take(sv.size() * sizeof(SightView));
    const size_t at_h = cur.take(M * sizeof(float)), at_out = cur.take((size_t)n * words * sizeof(uint32_t));
    if ((rc = sight_io(c, cur.next))) return rc;
    if (!he.empty() && !ps.sight_rows) HIP_TRY(hip_alloc(ps.sight_rows, (size_t)c->cfg.max_batch * sc.sectors.size() * sizeof(FsHeights)));
    if (!pe.empty() && !ps.sight_poses) HIP_TRY(hip_alloc(ps.sight_poses, (size_t)c->cfg.max_batch * M * sizeof(FsMobj)));
    const bool rows = !he.empty() || !pe.empty();
    HIP_TRY(c->sight.begin());
    c->sight_rows.measured = false;
    if (rows) HIP_TRY(c->sight_rows.begin());
    const hipStream_t xs = c->xstream.get();
    uint8_t *const d = ps.sight_io.get();
    SightMobjParams P{ps.sight_T, reinterpret_cast<const SightView *>(d + at_v), ps.sight_mobjs, reinterpret_cast<const float *>(d + at_h),
                      reinterpret_cast<uint32_t *>(d + at_out), (uint32_t)n, (uint32_t)M, (uint32_t)words, 1u};
    hipError_t e = hipMemcpyAsync(d + at_v, sv.data(), sv.size() * sizeof(SightView), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess) e = hipMemcpyAsync(d + at_h, mobj_height, M * sizeof(float), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess && !he.empty()) e = hipMemcpyAsync(d + at_he, he.data(), he.size() * sizeof(SectorEntry), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess && !pe.empty()) e = hipMemcpyAsync(d + at_pe, pe.data(), pe.size() * sizeof(PoseEntry), hipMemcpyHostToDevice, xs);
    if (e == hipSuccess)
        e = sight_queue_rows(c, xs, n, reinterpret_cast<const SectorEntry *>(d + at_he), he.size(), reinterpret_cast<const PoseEntry *>(d + at_pe), pe.size(), P.T, P.poses,
                             P.pose_frames);
    if (e == hipSuccess) e = launch_sight_mobjs(P, xs, c->sight.t0.get(), c->sight.t1.get());
    if (e == hipSuccess) e = hipMemcpyAsync(visible_out, d + at_out, (size_t)n * words * sizeof(uint32_t), hipMemcpyDeviceToHost, xs);
    if ((rc = finish(xs, e, "dg_sight_mobjs_device"))) return rc;     // before the staged inputs go and the caller reads, whatever was queued has run
    c->sight.end();
    if (rows) c->sight_rows.end();
    return DG_OK;
}

int dg_ctx_sight_kernel_ms(dg_ctx *c, float *rows_ms, float *sight_ms) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (!c->sight.measured) return set_err(DG_ERR_INVALID, "no dg_sight_device or dg_sight_mobjs_device call has launched yet");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (sight_ms) HIP_TRY(c->sight.elapsed(sight_ms));
    if (rows_ms) { *rows_ms = 0.0f; if (c->sight_rows.measured) HIP_TRY(c->sight_rows.elapsed(rows_ms)); }
    return DG_OK;
}

int dg_ctx_locate_walks(dg_ctx *c, dg_walk *const *walks, int n_walks) {
    if (!c || n_walks < 0 || (n_walks > 0 && !walks)) return set_err(DG_ERR_INVALID, "null argument");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded");
    for (int i = 0; i < n_walks; i++) {
        if (!walks[i]) return set_err(DG_ERR_INVALID, "null walk");
        if (walks[i]->sc != c->scene) return set_err(DG_ERR_INVALID, "a walk was created on another scene than the one uploaded");
    }
    // the walks still to locate, each once, and what they add up to
    std::vector<dg_walk *> todo;
    uint64_t probes = 0, entries = 0;
    for (int i = 0; i < n_walks; i++) {
        dg_walk *w = walks[i];
        if (w->located || w->queued) continue;
        w->queued = true;
        todo.push_back(w);
        probes += w->px.size();
        entries += w->pose.size();
    }
    for (dg_walk *w : todo) w->queued = false;
    if (todo.empty()) return DG_OK;
    if (probes > WALK_MAX_PROBES) return set_err(DG_ERR_CAPACITY, "more than 1 << 26 probes in one call");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const Scene &sc = *c->scene;
    HIP_TRY(side_stream(c->wstream));
    const hipStream_t ws = c->wstream.get();
    if (!c->per_scene.walk_tables) {
        TablePack t;
        const size_t nodes = t.add(sc.walk_nodes), leaves = t.add(sc.walk_leaves);
        DevPtr<uint8_t> d_tables;
        const hipError_t e = t.upload(d_tables);
        if (e != hipSuccess) return set_err(DG_ERR_HIP, std::string("walk tables: ") + hipGetErrorString(e));
        c->per_scene.walk_tables = std::move(d_tables);
        c->per_scene.walk_nodes = t.at<WalkNode>(nodes);
        c->per_scene.walk_leaves = t.at<WalkLeaf>(leaves);
    }
    // one slab: the probes of all walks, concatenated, go up in one copy; the floors come back in one
    const WalkLayout L = walk_layout((size_t)probes, (size_t)entries);
    std::vector<uint8_t> staged(L.upload);
    float *hx = reinterpret_cast<float *>(staged.data() + L.x), *hy = reinterpret_cast<float *>(staged.data() + L.y);
    uint8_t *hfirst = staged.data() + L.first;
    uint32_t *heot = reinterpret_cast<uint32_t *>(staged.data() + L.end_of_tic);
    size_t pi = 0, ei = 0;
    for (const dg_walk *w : todo) {
        const size_t np = w->px.size(), ne = w->pose.size();
        std::memcpy(hx + pi, w->px.data(), np * 4);
        std::memcpy(hy + pi, w->py.data(), np * 4);
        hfirst[pi] = 1;
        for (size_t t = 0; t < ne; t++) heot[ei + t] = (uint32_t)pi + w->end_of_tic[t];
        pi += np; ei += ne;
    }
    DevPtr<uint8_t> d_slab;
    HIP_TRY(hip_alloc(d_slab, L.total));
    uint8_t *const d = d_slab.get();
    WalkParams P{};
    P.nodes = c->per_scene.walk_nodes; P.leaves = c->per_scene.walk_leaves;
    P.x = reinterpret_cast<const float *>(d + L.x); P.y = reinterpret_cast<const float *>(d + L.y);
    P.first = d + L.first; P.end_of_tic = reinterpret_cast<const uint32_t *>(d + L.end_of_tic);
    P.value = reinterpret_cast<float *>(d + L.value); P.last = reinterpret_cast<uint32_t *>(d + L.last);
    P.sums = reinterpret_cast<uint32_t *>(d + L.sums); P.floors = reinterpret_cast<float *>(d + L.floors);
    P.root = (int32_t)sc.walk_nodes.size() - 1;
    P.n_probes = (uint32_t)probes; P.n_blocks = (uint32_t)walk_scan_blocks((size_t)probes); P.n_entries = entries;
    std::vector<float> floors((size_t)entries);
    hipError_t e = hipMemcpyAsync(d, staged.data(), L.upload, hipMemcpyHostToDevice, ws);
    if (e == hipSuccess) e = launch_walk_locate(P, ws);
    if (e == hipSuccess) e = hipMemcpyAsync(floors.data(), d + L.floors, (size_t)entries * 4, hipMemcpyDeviceToHost, ws);
    if (const int bad = finish(ws, e, "dg_ctx_locate_walks")) return bad;     // before d_slab and the staging go, whatever was queued has run
    ei = 0;
    for (dg_walk *w : todo) {
        w->floors.assign(floors.begin() + (ptrdiff_t)ei, floors.begin() + (ptrdiff_t)(ei + w->pose.size()));
        w->located = true;
        ei += w->pose.size();
    }
    return DG_OK;
}

}  // extern "C"
