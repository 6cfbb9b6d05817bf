// api_readback.cpp — the entry points of the C-ABI (include/doomgpu.h) that read what a slot's submission left: the eight readbacks of
// its frames and planes, and the calls that read one thing of a finished submission (dg_frame_checksums, dg_slot_mobj_poses,
// dg_slot_framebuffer, the four timing getters).  How a slot gets its submission, make_final and dg_wait: context.cpp.
//
// A readback is described once (Slot::Readback: full-size or reduced RGB24 frames, full-size or reduced planes, and where the box rows
// land), queued by one function (issue_readback) and finished by one (finish_readback: the box rows as dg_label_box).  Two drivers run
// it: read_now on the slot's own stream, done when the call returns, and read_later on the slot's copy stream behind ev_raster, as the
// slot's one pending readback (Slot::copy, copy_pending), which dg_wait or the slot's next submission completes.  The rules:
// - The slot's scratch (d_reduced) and its pinned box staging (h_rawboxes) belong to one reduced readback at a time.  A pending one owns
//   them until it is completed, so read_now completes it first (Copy::Complete) when its own readback is a reduced one too, and only
//   then.  Both buffers only grow, in reserve(), after a sync of both streams of the slot.
// - The full-size readbacks, the checksums and the getters need neither buffer and leave a pending readback alone (Copy::Leave): the
//   box rows of a synchronous dg_readback_labels land in memory of the call's own, never in h_rawboxes.
// - One readback is pending per slot, of any kind; read_later refuses a second.
// - Frames redone at make_final (a column-walk batch that overflowed) are newer than what a pending readback copied: make_final queues
//   it again (enqueue_copy) and finishes it exactly once; dg_upload_scene finishes that of a slot it only drained.
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "context.hpp"
#include "plane_reduce_kernels.hpp"
#include "reduce_kernels.hpp"

using namespace dg;

namespace {

// Frames [first, first + count) of what the slot holds, into an output that is there.
int check_range(const Slot &s, int first, int count, bool out = true, const char *what = "bad readback range") {
    if (!out || first < 0 || count < 0 || first + count > s.n_frames) return set_err(DG_ERR_INVALID, what);
    return DG_OK;
}

// The checked slot's submission made final, with the ctx's device current.
int settle(dg_ctx *c, Slot &s, Copy copy) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    return make_final(c, s, copy);
}

// Room for n elements in one of the slot's two readback buffers (buf, cap: the scratch d_reduced, the box staging h_rawboxes).  It only
// ever grows, and only when nothing of the slot can be using it: after a sync of the slot's streams.
template <class T, class Mem>
int grow(Slot &s, std::unique_ptr<T, Mem> &buf, size_t &cap, size_t n) {
    if (n <= cap) return DG_OK;
    HIP_TRY(hipStreamSynchronize(s.stream.get()));
    HIP_TRY(hipStreamSynchronize(s.copy_stream.get()));
    cap = 0;
    HIP_TRY(hip_alloc(buf, n * sizeof(T)));
    cap = n;
    return DG_OK;
}

// Where a reduced plane readback of `count` frames puts its outputs in the slot's scratch: the 16-bit planes first, every plane on a
// 256-byte boundary, whether it is asked for or not (the scratch is sized for all four).
struct PlaneScratch { size_t px, distance, id, kind, cls, total; };   // px: elements of one plane, byte offsets, bytes in all
PlaneScratch plane_scratch(const dg_ctx *c, const dg_plane_reduce_desc &d, int count) {
    const size_t px = (size_t)count * reduce_out_dim((uint32_t)c->cfg.width, d.fx) * reduce_out_dim((uint32_t)c->cfg.height, d.fy);
    SlabCursor cur;
    PlaneScratch p{};
    p.px = px;
    p.distance = cur.take(2 * px); p.id = cur.take(2 * px); p.kind = cur.take(px); p.cls = cur.take(px);
    p.total = cur.next;
    return p;
}

// What reduced readback r needs of the slot: room in its scratch, and for the box rows of reduced planes its pinned staging, where r
// then has them land.
int reserve(const dg_ctx *c, Slot &s, Slot::Readback &r) {
    if (!r.reduced) return DG_OK;
    int rc = grow(s, s.d_reduced, s.reduced_cap, r.planes ? plane_scratch(c, r.pdesc, r.count).total
                                                          : (size_t)r.count * reduce_frame_bytes((uint32_t)c->cfg.width, (uint32_t)c->cfg.height, r.desc));
    if (rc || !r.planes || !r.boxes) return rc;
    rc = grow(s, s.h_rawboxes, s.rawbox_cap, (size_t)r.count * s.per_scene.box_mobjs);
    r.raw = s.h_rawboxes.get();
    return rc;
}

// A plane readback on `stream`: the copies of the planes asked for — the slot's planes themselves, or dg_plane_nearest / dg_plane_point
// from them into the slot's scratch and that — and the frames' box rows to where r has them land.
int issue_plane_readback(dg_ctx *c, Slot &s, const Slot::Readback &r, hipStream_t stream) {
    const size_t W = (size_t)c->cfg.width, H = (size_t)c->cfg.height, at = (size_t)r.first * W * H;
    const BundleLayout L = s.layout(W, H);
    const uint8_t *const fb = s.d_fb.get();
    PlaneReduceSrc src{};                                  // the planes the slot holds, from frame `first` on
    if (s.holds(BUNDLE_DEPTH)) {
        src.distance = reinterpret_cast<const int16_t *>(fb + L.distance) + at;        // (DG_PLANE_NEAREST reads it whatever is asked for)
        src.kind = fb + L.kind + at;
    }
    if (s.holds(BUNDLE_LABELS)) {
        src.id = reinterpret_cast<const uint16_t *>(fb + L.id) + at;
        src.cls = fb + L.cls + at;
    }
    size_t px = (size_t)r.count * W * H;                   // elements of one plane over the count frames
    if (r.reduced) {
        const PlaneScratch sc = plane_scratch(c, r.pdesc, r.count);
        if (sc.total > s.reduced_cap) return set_err(DG_ERR_INVALID, "reduced readback: no scratch reserved");
        uint8_t *const out = s.d_reduced.get();
        PlaneReduceDst dst{};
        if (r.distance && src.distance) dst.distance = reinterpret_cast<int16_t *>(out + sc.distance);
        if (r.kind && src.kind) dst.kind = out + sc.kind;
        if (r.id && src.id) dst.id = reinterpret_cast<uint16_t *>(out + sc.id);
        if (r.cls && src.cls) dst.cls = out + sc.cls;
        if (dst.distance || dst.kind || dst.id || dst.cls) HIP_TRY(launch_plane_reduce(src, c->cfg.width, c->cfg.height, r.count, r.pdesc, dst, stream));
        src = PlaneReduceSrc{dst.distance, dst.kind, dst.id, dst.cls};
        px = sc.px;
    }
    if (r.distance && src.distance) HIP_TRY(hipMemcpyAsync(r.distance, src.distance, 2 * px, hipMemcpyDeviceToHost, stream));
    if (r.kind && src.kind) HIP_TRY(hipMemcpyAsync(r.kind, src.kind, px, hipMemcpyDeviceToHost, stream));
    if (r.id && src.id) HIP_TRY(hipMemcpyAsync(r.id, src.id, 2 * px, hipMemcpyDeviceToHost, stream));
    if (r.cls && src.cls) HIP_TRY(hipMemcpyAsync(r.cls, src.cls, px, hipMemcpyDeviceToHost, stream));
    const size_t n_boxes = (size_t)r.count * s.per_scene.box_mobjs;
    if (r.raw && n_boxes) HIP_TRY(hipMemcpyAsync(r.raw, s.per_scene.d_boxes.get() + (size_t)r.first * s.per_scene.box_mobjs, n_boxes * sizeof(LabelRawBox), hipMemcpyDeviceToHost, stream));
    return DG_OK;
}

// Readback r of the slot on `stream`: the D2H copy of the frames themselves, or dg_reduce into the slot's scratch and the copy of
// that, or the planes (issue_plane_readback).  The caller has ordered `stream` behind the slot's kernels and reserved what r needs.
int issue_readback(dg_ctx *c, Slot &s, const Slot::Readback &r, hipStream_t stream) {
    const size_t fsz = (size_t)3 * (size_t)c->cfg.width * (size_t)c->cfg.height;
    const uint8_t *const frames = s.d_fb.get() + (size_t)r.first * fsz;
    if (!r.reduced && !r.planes) {
        HIP_TRY(hipMemcpyAsync(r.out, frames, (size_t)r.count * fsz, hipMemcpyDeviceToHost, stream));
        return DG_OK;
    }
    if (r.count == 0) return DG_OK;
    if (r.planes) return issue_plane_readback(c, s, r, stream);
    const size_t bytes = (size_t)r.count * reduce_frame_bytes((uint32_t)c->cfg.width, (uint32_t)c->cfg.height, r.desc);
    if (bytes > s.reduced_cap) return set_err(DG_ERR_INVALID, "reduced readback: no scratch reserved");
    HIP_TRY(launch_reduce(frames, c->cfg.width, c->cfg.height, r.count, r.desc, s.d_reduced.get(), stream));
    HIP_TRY(hipMemcpyAsync(r.out, s.d_reduced.get(), bytes, hipMemcpyDeviceToHost, stream));
    return DG_OK;
}

// Now: readback r on the slot's own stream, done when this returns.
int read_now(dg_ctx *c, Slot &s, Slot::Readback r) {
    int rc = settle(c, s, r.reduced && s.copy_pending && s.copy.reduced ? Copy::Complete : Copy::Leave);
    if (rc) return rc;
    if ((rc = reserve(c, s, r))) return rc;
    if ((rc = issue_readback(c, s, r, s.stream.get()))) return rc;
    HIP_TRY(slot_sync(s));
    finish_readback(c, s, r);
    return DG_OK;
}

// Later: readback r becomes the slot's pending one.  nothing: the call is valid and has nothing to do.
int read_later(dg_ctx *c, Slot &s, Slot::Readback r, bool nothing = false) {
    if (s.copy_pending) return set_err(DG_ERR_INVALID, "the slot already has a readback in flight (dg_wait it first)");
    if (nothing) return DG_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    int rc = reserve(c, s, r);
    if (rc) return rc;
    s.copy = r;
    if ((rc = enqueue_copy(c, s))) return rc;
    s.copy_pending = true;
    return DG_OK;
}

Slot::Readback frame_readback(int first, int count, uint8_t *out, const dg_reduce_desc *desc = nullptr) {
    Slot::Readback r;
    r.first = first; r.count = count; r.out = out;
    if (desc) { r.reduced = true; r.desc = *desc; }
    return r;
}

Slot::Readback plane_readback(int first, int count, int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes,
                              const dg_plane_reduce_desc *desc = nullptr) {
    Slot::Readback r;
    r.first = first; r.count = count; r.planes = true;
    r.distance = distance; r.kind = kind; r.id = id; r.cls = cls; r.boxes = boxes;
    if (desc) { r.reduced = true; r.pdesc = *desc; }
    return r;
}

// What the four readbacks of RGB24 frames check alike, the reduced ones after their descriptor: the slot, that it holds colour frames,
// the frame range and the output.
int check_frame_readback(dg_ctx *c, int slot, const char *name, int first, int count, const uint8_t *out) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    const Slot &s = c->slots[(size_t)slot];
    if ((rc = refuse_no_colour(s, name))) return rc;
    return check_range(s, first, count, out != nullptr);
}

// What dg_readback_planes_reduced and its asynchronous twin check alike, in this order: the descriptor, the slot, what the slot holds
// against what is asked for, the frame range.  *nothing: the call is valid and has nothing to do.
int check_plane_readback(dg_ctx *c, int slot, const dg_plane_reduce_desc *desc, const Slot::Readback &r, bool *nothing) {
    if (!desc) return set_err(DG_ERR_INVALID, "null argument");
    if (!plane_reduce_desc_ok(*desc)) return set_err(DG_ERR_INVALID, "plane reduce descriptor: fx and fy in 1..16, a known rule, reserved 0");
    int rc = check_slot(c, slot);
    if (rc) return rc;
    const Slot &s = c->slots[(size_t)slot];
    if (!s.holds(BUNDLE_DEPTH) && !s.holds(BUNDLE_LABELS)) return set_err(DG_ERR_INVALID, "reduced planes: the slot holds neither depth nor label planes");
    if ((r.distance || r.kind) && !s.holds(BUNDLE_DEPTH)) return set_err(DG_ERR_INVALID, "reduced planes: the slot has no depth part (distance, kind)");
    if ((r.id || r.cls || r.boxes) && !s.holds(BUNDLE_LABELS)) return set_err(DG_ERR_INVALID, "reduced planes: the slot has no label part (id, cls, boxes)");
    if (desc->rule == DG_PLANE_NEAREST && !s.holds(BUNDLE_DEPTH)) return set_err(DG_ERR_INVALID, "reduced planes: DG_PLANE_NEAREST needs a slot with a depth part");
    if ((rc = check_range(s, r.first, r.count))) return rc;
    *nothing = r.count == 0 || !(r.distance || r.kind || r.id || r.cls || r.boxes);
    return DG_OK;
}

// The times of the bundle the slot has run, into the outputs that are there: setup and raster are the colour kernels' (the raster
// launch ends at ev_cend when dg_bundle_tiles follows it), tiles is dg_bundle_tiles'; 0 for a part the bundle does not have.
int bundle_times(const Slot &s, float *setup_ms, float *raster_ms, float *tiles_ms) {
    const bool colour = (s.bundle_what & BUNDLE_COLOUR) != 0, tiles = (s.bundle_what & (BUNDLE_DEPTH | BUNDLE_LABELS)) != 0;
    if (setup_ms) { *setup_ms = 0.0f; if (colour) HIP_TRY(hipEventElapsedTime(setup_ms, s.ev_start.get(), s.ev_setup.get())); }
    if (raster_ms) { *raster_ms = 0.0f; if (colour) HIP_TRY(hipEventElapsedTime(raster_ms, s.ev_rstart.get(), tiles ? s.ev_cend.get() : s.ev_raster.get())); }
    if (tiles_ms) { *tiles_ms = 0.0f; if (tiles) HIP_TRY(hipEventElapsedTime(tiles_ms, s.ev_tiles.get(), s.ev_raster.get())); }
    return DG_OK;
}

}  // namespace

// The calls that read the framebuffer slab as RGB24 frames, or run the colour kernels again: the slot has no colour part.  (An empty
// slot is the callers' to refuse.)
int dg::refuse_no_colour(const Slot &s, const char *what) {
    if (s.parts() == 0 || s.holds(BUNDLE_COLOUR)) return DG_OK;   // (a bundle's colour frames sit at the slab's base, as after a colour submission)
    if (s.holds_bundle()) return set_err(DG_ERR_INVALID, std::string(what) + ": the slot holds a bundle without a colour part (DG_BUNDLE_COLOUR)");
    if (s.holds(BUNDLE_LABELS)) return set_err(DG_ERR_INVALID, std::string(what) + ": the slot holds label planes, not RGB24 frames (dg_readback_labels)");
    return set_err(DG_ERR_INVALID, std::string(what) + ": the slot holds depth planes, not RGB24 frames (dg_readback_depth)");
}

// The slot's pending readback onto its copy stream, behind the slot's kernels.
int dg::enqueue_copy(dg_ctx *c, Slot &s) {
    HIP_TRY(hipStreamWaitEvent(s.copy_stream.get(), s.ev_raster.get(), 0));
    return issue_readback(c, s, s.copy, s.copy_stream.get());
}

// What is left to do on the host once readback r's copies have finished: the box rows in the form the caller sees.
void dg::finish_readback(const dg_ctx *c, const Slot &s, const Slot::Readback &r) {
    if (!r.boxes) return;
    const size_t n_boxes = (size_t)r.count * s.per_scene.box_mobjs;
    for (size_t i = 0; i < n_boxes; i++) {
        int32_t x0, y0, x1, y1;
        label_box_finish(r.raw[i], c->cfg.width, c->cfg.height, r.boxes[i].pixels, x0, y0, x1, y1);
        r.boxes[i].x0 = (int16_t)x0; r.boxes[i].y0 = (int16_t)y0; r.boxes[i].x1 = (int16_t)x1; r.boxes[i].y1 = (int16_t)y1;
    }
}

namespace {

// One kind of per-view rows (view_rows_core.h) of the slot's view submission, frames [first, first + count): what the kind's kernels
// wrote when the batch went through the seg walk with them, else the scene's row with the frame's kept entries on top — `host` puts
// one frame's there, by the host walker's rule.
template <class K, class Host>
int slot_rows(dg_ctx *c, int slot, int first, int count, typename K::Elem *out, const char *call, const RowRun<K> Slot::*run,
              const std::vector<typename K::Elem> Scene::*scene_rows, Host host) {
    using Elem = typename K::Elem;
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (s.phase == Slot::Phase::Empty || !s.from_views || !c->scene) return set_err(DG_ERR_STATE, std::string(call) + ": the slot holds no view submission");
    if ((rc = check_range(s, first, count, out != nullptr, "bad frame range"))) return rc;
    if (count == 0) return DG_OK;
    if ((rc = settle(c, s, Copy::Leave))) return rc;       // (a seg-walk batch redone as a whole is a host-list batch from here on)
    const Scene &sc = *c->scene;
    const std::vector<Elem> &loaded = sc.*scene_rows;
    const size_t n_items = loaded.size();
    if (n_items == 0) return DG_OK;
    if (s.seg_walk() && (s.*run).on()) {                   // the rows the kind's kernels wrote
        HIP_TRY(hipMemcpyAsync(out, (s.*run).P.rows + (size_t)first * n_items, (size_t)count * n_items * sizeof(Elem), hipMemcpyDeviceToHost, s.stream.get()));
        HIP_TRY(slot_sync(s));
        return DG_OK;
    }
    FrameArena &A = *c->arenas[0];
    for (int i = 0; i < count; i++) {
        Elem *row = out + (size_t)i * n_items;
        std::memcpy(row, loaded.data(), n_items * sizeof(Elem));
        host(sc, s, A, first + i, row);
    }
    return DG_OK;
}

// The time of the kind's kernels in the slot's last submission; 0 when it had none.
template <class K> int slot_rows_timing(dg_ctx *c, int slot, float *ms, const RowRun<K> Slot::*run) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!ms) return set_err(DG_ERR_INVALID, "null argument");
    Slot &s = c->slots[(size_t)slot];
    if (!s.has_run()) return set_err(DG_ERR_INVALID, "slot has not run yet");
    if ((rc = settle(c, s, Copy::Leave))) return rc;
    *ms = 0.0f;
    const RowRun<K> &r = s.*run;
    if (s.seg_walk() && r.on()) HIP_TRY(hipEventElapsedTime(ms, (r.from_start ? s.ev_start : r.t0).get(), r.t1.get()));
    return DG_OK;
}

}  // namespace

extern "C" {

int dg_readback(dg_ctx *c, int slot, int first, int count, uint8_t *out) {
    const int rc = check_frame_readback(c, slot, "dg_readback", first, count, out);
    return rc ? rc : read_now(c, c->slots[(size_t)slot], frame_readback(first, count, out));
}

int dg_readback_async(dg_ctx *c, int slot, int first, int count, uint8_t *out) {
    const int rc = check_frame_readback(c, slot, "dg_readback_async", first, count, out);
    return rc ? rc : read_later(c, c->slots[(size_t)slot], frame_readback(first, count, out));
}

int dg_readback_reduced(dg_ctx *c, int slot, int first, int count, const dg_reduce_desc *desc, uint8_t *out) {
    int rc = check_reduce_desc(desc);
    if (!rc) rc = check_frame_readback(c, slot, "dg_readback_reduced", first, count, out);
    if (rc || count == 0) return rc;
    return read_now(c, c->slots[(size_t)slot], frame_readback(first, count, out, desc));
}

int dg_readback_reduced_async(dg_ctx *c, int slot, int first, int count, const dg_reduce_desc *desc, uint8_t *out) {
    int rc = check_reduce_desc(desc);
    if (!rc) rc = check_frame_readback(c, slot, "dg_readback_reduced_async", first, count, out);
    return rc ? rc : read_later(c, c->slots[(size_t)slot], frame_readback(first, count, out, desc));
}

int dg_readback_depth(dg_ctx *c, int slot, int first, int count, int16_t *distance, uint8_t *kind) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (!s.holds(BUNDLE_DEPTH))                           // (a label slot included)
        return set_err(DG_ERR_INVALID, s.holds_bundle() ? "dg_readback_depth: the slot's bundle has no depth part (DG_BUNDLE_DEPTH)"
                                                        : "dg_readback_depth: the slot's last submission is not a depth submission");
    if ((rc = check_range(s, first, count))) return rc;
    if (count == 0) return DG_OK;
    return read_now(c, s, plane_readback(first, count, distance, kind, nullptr, nullptr, nullptr));
}

int dg_readback_labels(dg_ctx *c, int slot, int first, int count, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (!s.holds(BUNDLE_LABELS))
        return set_err(DG_ERR_INVALID, s.holds_bundle() ? "dg_readback_labels: the slot's bundle has no label part (DG_BUNDLE_LABELS)"
                                                        : "dg_readback_labels: the slot's last submission is not a label submission");
    if ((rc = check_range(s, first, count))) return rc;
    if (count == 0) return DG_OK;
    std::vector<LabelRawBox> raw(boxes ? (size_t)count * s.per_scene.box_mobjs : 0);      // (not the slot's staging: a pending readback may own it)
    Slot::Readback r = plane_readback(first, count, nullptr, nullptr, id, cls, boxes);
    r.raw = raw.data();
    return read_now(c, s, r);
}

int dg_readback_planes_reduced(dg_ctx *c, int slot, int first, int count, const dg_plane_reduce_desc *desc,
                               int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    const Slot::Readback r = plane_readback(first, count, distance, kind, id, cls, boxes, desc);
    bool nothing = false;
    const int rc = check_plane_readback(c, slot, desc, r, &nothing);
    if (rc || nothing) return rc;
    return read_now(c, c->slots[(size_t)slot], r);
}

int dg_readback_planes_reduced_async(dg_ctx *c, int slot, int first, int count, const dg_plane_reduce_desc *desc,
                                     int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    const Slot::Readback r = plane_readback(first, count, distance, kind, id, cls, boxes, desc);
    bool nothing = false;
    const int rc = check_plane_readback(c, slot, desc, r, &nothing);
    if (rc) return rc;
    return read_later(c, c->slots[(size_t)slot], r, nothing);
}

int dg_frame_checksums(dg_ctx *c, int slot, int first, int count, uint64_t *out) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if ((rc = refuse_no_colour(s, "dg_frame_checksums"))) return rc;
    if ((rc = check_range(s, first, count, out != nullptr, "bad frame range"))) return rc;
    if (count == 0) return DG_OK;
    if ((rc = settle(c, s, Copy::Leave))) return rc;       // (the kernels run on the ctx's kernel stream: the copy below is not ordered behind them by its stream)
    const size_t fsz = (size_t)3 * (size_t)c->cfg.width * (size_t)c->cfg.height;
    unsigned long long *d_sum = c->d_checksums.get();      // max_batch entries, allocated at dg_create
    hipError_t e = hipMemsetAsync(d_sum, 0, (size_t)count * 8, s.stream.get());
    if (e == hipSuccess) e = launch_checksums(s.d_fb.get() + (size_t)first * fsz, fsz, count, d_sum, s.stream.get());
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_sum, (size_t)count * 8, hipMemcpyDeviceToHost, s.stream.get());
    if (e == hipSuccess) e = slot_sync(s);
    if (e != hipSuccess) return set_err(DG_ERR_HIP, std::string("dg_frame_checksums: ") + hipGetErrorString(e));
    return DG_OK;
}

int dg_slot_mobj_poses(dg_ctx *c, int slot, int first, int count, dg_mobj_placed *out) {
    static_assert(sizeof(dg_mobj_placed) == sizeof(FsMobj) && offsetof(dg_mobj_placed, sector) == offsetof(FsMobj, sector), "dg_mobj_placed / FsMobj");
    return slot_rows<PoseRows>(c, slot, first, count, reinterpret_cast<FsMobj *>(out), "dg_slot_mobj_poses", &Slot::pose_run, &Scene::fs_mobjs,
                               [](const Scene &sc, const Slot &s, FrameArena &A, int frame, FsMobj *row) {      // (Walker::mobj_placed)
                                   const dg_view_poses *vp = s.kept.at(frame).poses;
                                   if (!vp) return;
                                   (void)resolve_view_poses(sc, *vp, A.poses);
                                   for (const dg_mobj_pose &p : A.poses.out) row[p.mobj] = FsMobj{p.x, p.y, p.angle, sc.sector_from_vertex(p.x, p.y)};
                                   A.poses.release();
                               });
}

int dg_slot_sector_heights(dg_ctx *c, int slot, int first, int count, int16_t *out) {
    return slot_rows<HeightRows>(c, slot, first, count, reinterpret_cast<FsHeights *>(out), "dg_slot_sector_heights", &Slot::height_run, &Scene::fs_heights,
                                 [](const Scene &sc, const Slot &s, FrameArena &A, int frame, FsHeights *row) {
                                     const dg_view_sectors *vs = s.kept.at(frame).sectors;
                                     if (!vs) return;
                                     (void)resolve_view_sectors(sc, *vs, A.heights);
                                     for (const dg_sector_heights &h : A.heights.out) sector_row_place(row, h.sector, h.floor_height, h.ceiling_height);
                                     A.heights.release();
                                 });
}

int dg_slot_sector_height_timing(dg_ctx *c, int slot, float *ms) { return slot_rows_timing(c, slot, ms, &Slot::height_run); }

int dg_slot_sector_flats(dg_ctx *c, int slot, int first, int count, int32_t *out) {
    return slot_rows<FlatRows>(c, slot, first, count, reinterpret_cast<FsFlats *>(out), "dg_slot_sector_flats", &Slot::flat_run, &Scene::fs_flats,
                               [](const Scene &sc, const Slot &s, FrameArena &A, int frame, FsFlats *row) {
                                   const dg_view_surfaces *vs = s.kept.at(frame).surfaces;
                                   if (!vs) return;
                                   (void)resolve_view_surfaces(sc, nullptr, *vs, frame, A.sides, A.flats);
                                   for (const FlatEntry &e : A.flats.out) flat_row_place(row, e.sector, e.flats);
                               });
}

int dg_slot_surface_timing(dg_ctx *c, int slot, float *ms) { return slot_rows_timing(c, slot, ms, &Slot::flat_run); }

int dg_slot_framebuffer(dg_ctx *c, int slot, void **p) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!p) return set_err(DG_ERR_INVALID, "null argument");
    *p = c->slots[(size_t)slot].d_fb.get();
    return DG_OK;
}

int dg_slot_mobj_pose_timing(dg_ctx *c, int slot, float *ms) { return slot_rows_timing(c, slot, ms, &Slot::pose_run); }

int dg_slot_label_timing(dg_ctx *c, int slot, float *tiles_ms, float *boxes_ms) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (s.front_end != DG_FE_LABELS || !s.has_run()) return set_err(DG_ERR_INVALID, "dg_slot_label_timing: the slot's last submission is not a label submission that ran");
    if ((rc = settle(c, s, Copy::Leave))) return rc;
    if (tiles_ms) HIP_TRY(hipEventElapsedTime(tiles_ms, s.ev_rstart.get(), s.ev_setup.get()));
    if (boxes_ms) HIP_TRY(hipEventElapsedTime(boxes_ms, s.ev_setup.get(), s.ev_raster.get()));
    return DG_OK;
}

int dg_slot_bundle_timing(dg_ctx *c, int slot, float *setup_ms, float *raster_ms, float *tiles_ms) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (!s.holds_bundle() || !s.has_run()) return set_err(DG_ERR_INVALID, "dg_slot_bundle_timing: the slot's last submission is not a bundle that ran");
    rc = settle(c, s, Copy::Leave);
    return rc ? rc : bundle_times(s, setup_ms, raster_ms, tiles_ms);
}

int dg_slot_timing(dg_ctx *c, int slot, dg_timing *out) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!out) return set_err(DG_ERR_INVALID, "null argument");
    Slot &s = c->slots[(size_t)slot];
    if (!s.has_run()) return set_err(DG_ERR_INVALID, "slot has not run yet");
    if ((rc = settle(c, s, Copy::Leave))) return rc;
    std::memset(out, 0, sizeof *out);
    out->front_end = s.front_end;
    if (s.front_end == DG_FE_BUNDLE) {                    // setup_ms / raster_ms: the colour kernels (0 without colour); total_ms: first kernel's start .. last kernel's end
        if ((rc = bundle_times(s, &out->setup_ms, &out->raster_ms, nullptr))) return rc;
        HIP_TRY(hipEventElapsedTime(&out->total_ms, (s.bundle_what & BUNDLE_COLOUR) ? s.ev_start.get() : s.ev_tiles.get(), s.ev_raster.get()));
    } else if (s.timed_front_half()) {
        HIP_TRY(hipEventElapsedTime(&out->raster_ms, s.ev_rstart.get(), s.ev_raster.get()));
        HIP_TRY(hipEventElapsedTime(&out->setup_ms, s.ev_start.get(), s.ev_setup.get()));
        HIP_TRY(hipEventElapsedTime(&out->total_ms, s.ev_start.get(), s.ev_raster.get()));
    } else {
        HIP_TRY(hipEventElapsedTime(&out->raster_ms, s.ev_rstart.get(), s.ev_raster.get()));
        out->total_ms = out->raster_ms;
    }
    out->n_spans = s.n_spans; out->n_frames = (uint64_t)s.n_frames; out->covered_pixels = s.covered;
    out->host_ms = s.host_ms; out->list_bytes = s.list_bytes;
    out->n_walls = s.n_walls; out->n_planes = s.n_planes;
    return DG_OK;
}

}  // extern "C"
