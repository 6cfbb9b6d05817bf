// context.cpp — dg_ctx: one GPU's resident scene, per-slot list slabs / framebuffer slabs / streams, the batch builders that run on
// the host thread pool (pool.hpp), and a slot's way from one submission to the next (Slot::Phase, take_slot, make_final).  Implements
// the entry points of the C-ABI (include/doomgpu.h) that give a slot of a dg_ctx its submission or wait for it; those that read what
// the submission left (the readbacks, the checksums, the timing getters) are in api_readback.cpp, those that run on a stream of the
// ctx's own and return when done in api_device.cpp, those that need no GPU in api_scene.cpp.  Slot and dg_ctx themselves: context.hpp;
// the owners of memory, streams and events and TablePack: hip_mem.hpp.
//
// HBM layout (sized once at dg_create for 288 GB parts: nothing is reallocated on the submit path):
//   scene   : palette 1 KB | texel index plane | texel opacity plane | flats (4 KB each)      immutable per map
//   per slot: list slab  [DevFrame x F | col_off x F*(W+1) | DevWallRec.. | DevPlaneRec.. | DevSpan..]  one H2D copy
//             rspan slab DevRSpan 32 B per span (device-only, written by dg_setup_spans, walked by dg_raster_tiles)
//             framebuffer slab  F x 3*W*H bytes RGB24 (the reference's Pixels.pixels, one per frame)
//             DG_FE_DEVICE: record slab [DevFrame x F | FeFrame x F | FePart.. | FeSprite.. | behind bits.. | sky slot -> part.. | column bins..] (one H2D copy),
//             col_off F*(W+1) written by dg_fe_finalize, 2F status words (overflow flags, span totals)
//             2-D map view: the arrow lines of the batch (MapSeg x 3F) at the start of the list slab
//             depth frames (DG_FE_DEPTH): the host lists in the list slab; the framebuffer slab holds int16 distance[F][H][W], then uint8 kind[F][H][W]
//             label frames (DG_FE_LABELS): likewise, the framebuffer slab holds uint16 id[F][H][W], then uint8 cls[F][H][W]; the owner tags
//             parallel to the list slab's wall records and the box table [max_batch][map objects] are buffers of the slot's own,
//             allocated by its first label submission (the box table again after dg_upload_scene)
//             bundles (DG_FE_BUNDLE): the host lists in the list slab; the framebuffer slab holds the requested parts, RGB24 frames first,
//             as slab_layout.h's bundle_layout places them; owner tags and box table as for label frames
//   per ctx : 2-D map view layer 3*W*H bytes RGB24 (allocated by the first map submission, rebuilt after every dg_upload_scene)
//             DG_FE_DEVICE column scratch [F][slot][W]: compact spans 16 B (48 slots), wall-record columns 8 B (48 slots),
//             counts, sky event bits — shared by the slots because their kernels run back to back
// The exact order and offsets of every slab's pieces: slab_layout.h.
#include <hip/hip_runtime_api.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "context.hpp"
#include "ego_host.hpp"
#include "ego_kernels.hpp"
#include "floor_map_host.hpp"
#include "floor_map_kernels.hpp"
#include "map_things_host.hpp"
#include "map_things_kernels.hpp"
#include "explored_cover.hpp"
#include "explored_kernels.hpp"
#include "map_kernels.hpp"

using namespace dg;

hipError_t dg::slot_sync(Slot &s) {
    if (s.raster_recorded) { const hipError_t e = hipEventSynchronize(s.ev_raster.get()); if (e != hipSuccess) return e; }
    return hipStreamSynchronize(s.stream.get());
}

int dg::check_slot(dg_ctx *c, int slot) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    if (slot < 0 || slot >= (int)c->slots.size()) return set_err(DG_ERR_INVALID, "slot out of range");
    return DG_OK;
}

namespace {

// CPUs' worth of run time the container allows this process (cgroup v2 cpu.max, v1 cfs quota), rounded up; 0 = no limit / unknown.
int cgroup_cpu_quota() {
    long long quota = -1, period = 0;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
        std::fclose(f);
    } else {
        if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(g, "%lld", &quota) != 1) quota = -1; std::fclose(g); }
        if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(g, "%lld", &period) != 1) period = 0; std::fclose(g); }
    }
    if (quota <= 0 || period <= 0) return 0;
    return (int)((quota + period - 1) / period);
}

// What every batch builder checks first: a scene is resident, the batch fits, the resident texels are still the scene's.
int check_batch(const dg_ctx *c, int n) {
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    if (c->scene->texel_idx.size() != c->uploaded_texels) return set_err(DG_ERR_INVALID, "the scene decoded new bitmaps since dg_upload_scene: upload it again");
    if (c->scene->flat_pool.size() != c->uploaded_flats || c->scene->anim.size() != c->uploaded_anims) return set_err(DG_ERR_INVALID, "the scene loaded new flats since dg_upload_scene: upload it again");
    return DG_OK;
}

// One binned frame into list slab `h` laid out as L: frame i of the batch, its records at the bases its header names.
void pack_binned(uint8_t *h, const ListLayout &L, const BinnedFrame &bf, size_t i, size_t W) {
    std::memcpy(h + L.frames + i * sizeof(DevFrame), &bf.hdr, sizeof(DevFrame));
    std::memcpy(h + L.col_off + i * (W + 1) * 4, bf.col_off.data(), (W + 1) * 4);
    if (!bf.walls.empty()) std::memcpy(h + L.walls + (size_t)bf.hdr.wall_base * sizeof(DevWallRec), bf.walls.data(), bf.walls.size() * sizeof(DevWallRec));
    if (!bf.planes.empty()) std::memcpy(h + L.planes + (size_t)bf.hdr.plane_base * sizeof(DevPlaneRec), bf.planes.data(), bf.planes.size() * sizeof(DevPlaneRec));
    if (!bf.spans.empty()) std::memcpy(h + L.spans + (size_t)bf.hdr.span_base * sizeof(DevSpan), bf.spans.data(), bf.spans.size() * sizeof(DevSpan));
}

// ... and the rasteriser's list pointers into the device copy `d` of such a slab.
void point_at_lists(RasterParams &P, const uint8_t *d, const ListLayout &L) {
    P.frames = reinterpret_cast<const DevFrame *>(d + L.frames);
    P.col_off = reinterpret_cast<const uint32_t *>(d + L.col_off);
    P.walls = reinterpret_cast<const DevWallRec *>(d + L.walls);
    P.planes = reinterpret_cast<const DevPlaneRec *>(d + L.planes);
    P.spans = reinterpret_cast<const DevSpan *>(d + L.spans);
}

// The part of slot.P that is the same whoever wrote the lists.
void fill_raster_params(dg_ctx *c, Slot &s, int n) {
    RasterParams &P = s.P;
    P.scene = c->dscene;
    P.k = c->dk;
    P.rspans = s.d_rspans.get();
    P.fb = s.d_fb.get();
    P.row_tab = c->d_row_tab.get();
    P.n_frames = n;
}

// One array of device slab `d` into a kernel parameter, and the walk's nine record arrays of a record slab laid out as L into P: FeLayout
// and FsLayout name those pieces alike, and so do FeParams, which reads them, and FsParams, which writes them.
template <class T> void point_at(T *&p, uint8_t *d, size_t off) { p = reinterpret_cast<T *>(d + off); }
template <class Params, class Layout> void point_at_records(Params &P, uint8_t *d, const Layout &L) {
    point_at(P.fframes, d, L.fframes); point_at(P.parts, d, L.parts); point_at(P.sprites, d, L.sprites);
    point_at(P.behind, d, L.behind); point_at(P.sky_parts, d, L.sky);
    point_at(P.bin_off, d, L.bin_off); point_at(P.sbin_off, d, L.sbin_off); point_at(P.bin_parts, d, L.bins); point_at(P.sbin_sprites, d, L.sbins);
}

uint32_t fe_span_stride(const dg_ctx *c) { return (uint32_t)(c->span_cap_per_batch / (size_t)c->cfg.max_batch); }

// The part of slot.FP / slot.P that does not depend on who wrote the records (the host walker or the device seg walk), given F.frames.
void fill_walk_params(dg_ctx *c, Slot &s, int n) {
    FeParams &F = s.FP;
    F.scene = c->dscene;
    F.k = c->dk;
    F.cspans = c->d_fe_cspans.get(); F.recs = c->d_fe_recs.get(); F.cnt = c->d_fe_cnt.get();
    F.events = s.d_events;
    F.flags = s.d_flags.get();
    F.host_flags = s.h_status.get(); F.totals = s.h_status.get() + c->cfg.max_batch;  // pinned host memory, written by dg_fe_scan with plain stores
    F.col_off = s.d_fe_coloff.get(); F.rspans = s.d_rspans.get();
    F.n_frames = n; F.span_stride = fe_span_stride(c); F.w64 = (uint32_t)((c->cfg.width + 63) / 64); F.col_slots = c->fe_col_slots;
    fill_raster_params(c, s, n);
    s.P.frames = F.frames;
    s.P.col_off = s.d_fe_coloff.get();
    s.P.walls = nullptr; s.P.planes = nullptr; s.P.spans = nullptr;
}

// Build + bin the lists of n views in parallel, pack them into the slot's pinned slab, fill slot.P.  fe: what the submission is described
// as — DG_FE_HOST, DG_FE_DEPTH when dg_depth_tiles will walk the lists, DG_FE_LABELS when dg_label_tiles will, or DG_FE_BUNDLE.  A label
// submission, and a bundle that says so (want_owners), needs owner tags: the tags of the wall records then go into the slot's owner array
// as well (the caller has allocated it), from given_owners[i] for the caller's lists.
int build_batch_host(dg_ctx *c, Slot &s, const dg_view *views, const dg_frame_lists *given, int n, const BatchInputs &in, int32_t fe = DG_FE_HOST,
                     const uint32_t *const *given_owners = nullptr, bool want_owners = false) {
    const auto t0 = std::chrono::steady_clock::now();
    if (const int bad = check_batch(c, n)) return bad;
    const Scene &sc = *c->scene;
    const int W = c->cfg.width, H = c->cfg.height;
    std::vector<int> rc((size_t)n, 0);
    std::vector<std::string> errs((size_t)n);
    const bool labels = fe == DG_FE_LABELS || want_owners;         // this submission needs owner tags
    if (labels && c->label_tags.size() < (size_t)n) c->label_tags.resize((size_t)n);
    c->pool->parallel_for(n, [&](int i, int wid) {
        BinnedFrame &bf = c->binned[(size_t)i];
        if (given) {
            dg_frame_lists fl = given[i];
            fill_view_trig(fl.view);
            rc[(size_t)i] = bin_frame(sc, c->fk, fl, bf, errs[(size_t)i]);
            if (labels && !rc[(size_t)i]) rc[(size_t)i] = wall_owners(sc, fl, given_owners[i], c->label_tags[(size_t)i], errs[(size_t)i]);
        } else {
            dg_view v = views[i];
            fill_view_trig(v);
            dg_frame_lists fl;
            rc[(size_t)i] = build_frame_lists(sc, W, H, v, *c->arenas[(size_t)wid], fl, errs[(size_t)i], in.at(i), &c->fx);
            if (!rc[(size_t)i]) rc[(size_t)i] = bin_frame(sc, c->fk, fl, bf, errs[(size_t)i]);
            if (labels && !rc[(size_t)i]) rc[(size_t)i] = wall_owners(sc, fl, c->arenas[(size_t)wid]->owners.data(), c->label_tags[(size_t)i], errs[(size_t)i]);
        }
    });
    for (int i = 0; i < n; i++)
        if (rc[(size_t)i]) return set_err(rc[(size_t)i], "frame " + std::to_string(i) + ": " + errs[(size_t)i]);

    // prefix sums -> bases
    uint64_t spans = 0, walls = 0, planes = 0, covered = 0;
    uint32_t max_spans = 0;
    for (int i = 0; i < n; i++) {
        BinnedFrame &bf = c->binned[(size_t)i];
        bf.hdr.span_base = (uint32_t)spans; bf.hdr.wall_base = (uint32_t)walls; bf.hdr.plane_base = (uint32_t)planes;
        spans += bf.spans.size(); walls += bf.walls.size(); planes += bf.planes.size(); covered += bf.covered_pixels;
        max_spans = std::max<uint32_t>(max_spans, (uint32_t)bf.spans.size());
    }
    if (spans > c->span_cap_per_batch || walls > c->wall_cap_per_batch || planes > c->plane_cap_per_batch)
        return set_err(DG_ERR_CAPACITY, "frame lists exceed the slot's list slab");
    const ListLayout L = list_layout((size_t)n, (size_t)W, walls, planes, spans);
    if (L.total > s.lists_cap) return set_err(DG_ERR_CAPACITY, "list slab too small");
    c->pool->parallel_for(n, [&](int i, int) {
        pack_binned(s.h_lists.get(), L, c->binned[(size_t)i], (size_t)i, (size_t)W);
        const std::vector<uint32_t> *tags = labels ? &c->label_tags[(size_t)i] : nullptr;      // (as many as the frame has wall records)
        if (tags && !tags->empty()) std::memcpy(s.h_owners.get() + c->binned[(size_t)i].hdr.wall_base, tags->data(), tags->size() * sizeof(uint32_t));
    });
    fill_raster_params(c, s, n);
    point_at_lists(s.P, s.d_lists.get(), L);
    s.describe(fe, n, L.total, walls, planes);
    s.max_spans = max_spans; s.n_spans = spans; s.covered = covered;
    s.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(hipMemcpyAsync(s.d_lists.get(), s.h_lists.get(), L.total, hipMemcpyHostToDevice, s.stream.get()));
    if (labels && walls) HIP_TRY(hipMemcpyAsync(s.d_owners.get(), s.h_owners.get(), walls * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream.get()));
    return DG_OK;
}

// DG_FE_DEVICE: build the per-seg / per-sprite records of n views in parallel, pack them into the slot's record slab,
// fill slot.FP / slot.P.  Returns kPartsUnsupported when the batch has to go through build_batch_host instead.
int build_batch_fe(dg_ctx *c, Slot &s, const dg_view *views, int n, const BatchInputs &in) {
    const auto t0 = std::chrono::steady_clock::now();
    if (const int bad = check_batch(c, n)) return bad;
    const Scene &sc = *c->scene;
    const int W = c->cfg.width, H = c->cfg.height;
    std::vector<int> rc((size_t)n, 0);
    std::vector<std::string> errs((size_t)n);
    c->pool->parallel_for(n, [&](int i, int wid) {
        FrameArena &A = *c->arenas[(size_t)wid];
        FeFrameOut &o = c->fe_out[(size_t)i];
        dg_view v = views[i];
        fill_view_trig(v);
        rc[(size_t)i] = build_frame_parts(sc, W, H, v, A, errs[(size_t)i], in.at(i), &c->fx);
        if (rc[(size_t)i]) return;
        o.parts.swap(A.parts); o.sprites.swap(A.sprites); o.behind.swap(A.behind); o.sky_parts.swap(A.sky_parts);
        o.bin_off.swap(A.bin_off); o.bin_parts.swap(A.bin_parts); o.sbin_off.swap(A.sbin_off); o.sbin_sprites.swap(A.sbin_sprites);
        o.behind_words = A.behind_words; o.n_sky_slots = A.n_sky_slots;
        o.hdr = make_frame_header(v);
    });
    for (int i = 0; i < n; i++) {
        if (rc[(size_t)i] == kPartsUnsupported) return kPartsUnsupported;
        if (rc[(size_t)i]) return set_err(rc[(size_t)i], "frame " + std::to_string(i) + ": " + errs[(size_t)i]);
    }
    uint64_t parts = 0, sprites = 0, behind = 0, skies = 0, bins = 0, sbins = 0;
    uint32_t max_sky = 0;
    std::vector<FeFrame> ffs((size_t)n);
    for (int i = 0; i < n; i++) {
        const FeFrameOut &o = c->fe_out[(size_t)i];
        if (o.n_sky_slots > FE_MAX_SKY_SLOTS) return kPartsUnsupported;
        ffs[(size_t)i] = FeFrame{(uint32_t)parts, (uint32_t)o.parts.size(), (uint32_t)sprites, (uint32_t)o.sprites.size(), (uint32_t)behind,
                                 o.behind_words, o.n_sky_slots, (uint32_t)skies, (uint32_t)bins, (uint32_t)sbins, {0u, 0u}};
        parts += o.parts.size(); sprites += o.sprites.size(); behind += o.behind.size(); skies += o.n_sky_slots;
        bins += o.bin_parts.size(); sbins += o.sbin_sprites.size();
        max_sky = std::max(max_sky, o.n_sky_slots);
    }
    if (parts > c->fe_part_cap || sprites > c->fe_sprite_cap || behind > c->fe_behind_cap || bins > c->fe_bin_cap || sbins > c->fe_sbin_cap)
        return kPartsUnsupported;
    const size_t nb1 = fe_bin_offsets((size_t)W), groups = fe_col_groups((size_t)W);
    const uint32_t span_stride = fe_span_stride(c);
    const FeLayout L = fe_layout((size_t)n, (size_t)W, parts, sprites, behind, skies, bins, sbins);
    if (L.total > c->fe_slab_cap) return kPartsUnsupported;
    uint8_t *const h = s.h_fe.get();
    {   // launch order of dg_fe_columns: heaviest workgroup first (weight = its longest bin: parts + 2 x sprites), counting sort
        std::vector<uint32_t> weight((size_t)n * groups), start(258, 0);
        for (int i = 0; i < n; i++) {
            const FeFrameOut &o = c->fe_out[(size_t)i];
            for (size_t g = 0; g < groups; g++) {
                uint32_t w = 0;
                for (size_t b = 4 * g; b < std::min(4 * g + 4, nb1 - 1); b++)
                    w = std::max(w, (o.bin_off[b + 1] - o.bin_off[b]) + 2u * (o.sbin_off[b + 1] - o.sbin_off[b]));
                w = 255u - std::min(w, 255u);                        // heaviest = smallest key
                weight[(size_t)i * groups + g] = w;
                start[w + 1]++;
            }
        }
        for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
        uint32_t *order = reinterpret_cast<uint32_t *>(h + L.order);
        for (size_t it = 0; it < weight.size(); it++) order[start[weight[it]]++] = (uint32_t)it;
    }
    c->pool->parallel_for(n, [&](int i, int) {
        FeFrameOut &o = c->fe_out[(size_t)i];
        const FeFrame &ff = ffs[(size_t)i];
        o.hdr.span_base = (uint32_t)i * span_stride;
        std::memcpy(h + L.frames + (size_t)i * sizeof(DevFrame), &o.hdr, sizeof(DevFrame));
        std::memcpy(h + L.fframes + (size_t)i * sizeof(FeFrame), &ff, sizeof(FeFrame));
        if (!o.parts.empty()) std::memcpy(h + L.parts + (size_t)ff.part_base * sizeof(FePart), o.parts.data(), o.parts.size() * sizeof(FePart));
        if (!o.sprites.empty()) std::memcpy(h + L.sprites + (size_t)ff.sprite_base * sizeof(FeSprite), o.sprites.data(), o.sprites.size() * sizeof(FeSprite));
        if (!o.behind.empty()) std::memcpy(h + L.behind + (size_t)ff.behind_base * 4, o.behind.data(), o.behind.size() * 4);
        if (!o.sky_parts.empty()) std::memcpy(h + L.sky + (size_t)ff.sky_base * 4, o.sky_parts.data(), o.sky_parts.size() * 4);
        std::memcpy(h + L.bin_off + (size_t)i * nb1 * 4, o.bin_off.data(), nb1 * 4);
        std::memcpy(h + L.sbin_off + (size_t)i * nb1 * 4, o.sbin_off.data(), nb1 * 4);
        if (!o.bin_parts.empty()) std::memcpy(h + L.bins + (size_t)ff.bin_base * 2, o.bin_parts.data(), o.bin_parts.size() * 2);
        if (!o.sbin_sprites.empty()) std::memcpy(h + L.sbins + (size_t)ff.sbin_base * 2, o.sbin_sprites.data(), o.sbin_sprites.size() * 2);
    });
    uint8_t *const d = s.d_fe.get();
    FeParams &F = s.FP;
    point_at(F.frames, d, L.frames);
    point_at_records(F, d, L);
    F.max_sky_slots = max_sky; F.gap_waves = 0;
    point_at(F.order, d, L.order); F.order_cnt = nullptr;
    fill_walk_params(c, s, n);
    s.describe(DG_FE_DEVICE, n, L.total, parts, sprites);
    s.views.assign(views, views + n);
    s.snapshot_scene(sc);
    s.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n >= 64 && !in.any()) c->fe_auto.host_batch((double)s.host_ms, n);      // DG_FE_AUTO's measurement of the host side
    HIP_TRY(hipMemcpyAsync(s.d_fe.get(), s.h_fe.get(), L.total, hipMemcpyHostToDevice, s.stream.get()));
    return DG_OK;
}

// DG_FE_DEVICE_SEGS: the scene's per-seg / per-sprite tables and BSP tables (Scene::rebuild_fs_tables) in one device allocation, the
// tables of the effects that are on in one each, and the per-batch scratch of the seg walk, whose size follows the scene (segs, leaves).
void drop_fs_scene(dg_ctx *c) { c->d_fs_scene.reset(); c->d_fs_scratch.reset(); c->d_wall_fx.reset(); c->d_light_fx.reset(); c->d_mobj_fx.reset(); }
// One kind of per-view rows at dg_upload_scene: `proto` becomes the scene side of its kernels' arguments, and every slot gets the
// kind's buffers.  scene_rows null: the scene has no such rows — no proto, no buffers.  A slot whose buffers cannot be had stays
// without, and sends its batches that carry the kind through the host walker (build_batch_fs).
template <class K>
void upload_view_rows(dg_ctx *c, ViewRowParams<K> &proto, RowBuffers<K> Slot::PerScene::*buffers, const typename K::Elem *scene_rows, size_t n_items,
                      const typename K::Ctx &ctx = {}) {
    proto = ViewRowParams<K>{};
    for (Slot &s : c->slots) s.per_scene.*buffers = {};
    if (!scene_rows) return;
    proto.scene_rows = scene_rows; proto.n_items = (uint32_t)n_items; proto.ctx = ctx;
    const ViewRowLayout L = view_row_layout<K>((size_t)c->cfg.max_batch, n_items);
    for (Slot &s : c->slots) (s.per_scene.*buffers).alloc(L);
}
int upload_fs_scene(dg_ctx *c, const Scene &sc) {
    drop_fs_scene(c);
    c->fs_fx = FsFx{};
    const WallFx &wfx = c->fx.wall;
    const LightFx &lfx = c->fx.light;
    const MobjFx &mfx = c->fx.mobj;
    if (wfx.on()) {                                     // the wall effects' tables: only for a scene that has them on (dg_wfx_* read them)
        TablePack t;
        const size_t seg = t.add(wfx.seg), lists = t.add(wfx.lists);
        HIP_TRY(t.upload(c->d_wall_fx));
        c->fs_fx = FsFx{t.at<FsSegFx>(seg), t.at<FsAnim>(lists)};
    }
    c->lfx_proto = LfxRows{};
    if (lfx.on()) {                                     // the light effects' records and tables: only for a scene that has them on (dg_light_rows reads them)
        TablePack t;
        const size_t recs = t.add(lfx.recs), rec_of = t.add(lfx.rec_of), tab = t.add(lfx.tab);
        HIP_TRY(t.upload(c->d_light_fx));
        c->lfx_proto.recs = t.at<LfxRec>(recs);
        c->lfx_proto.rec_of = t.at<int32_t>(rec_of);
        c->lfx_proto.tab = t.at<uint32_t>(tab);
        c->lfx_proto.seed = lfx.seed;
        c->lfx_proto.n_sectors = (uint32_t)lfx.rec_of.size();
    }
    c->mfx_proto = MfxRows{};
    if (mfx.on()) {                                     // the map-object thinkers' tables: only for a scene that has them on (dg_mobj_rows reads them)
        TablePack t;
        const size_t steps = t.add(mfx.steps), chains = t.add(mfx.chains), types = t.add(mfx.types), type_of = t.add(mfx.type_of), events = t.add(mfx.events);
        HIP_TRY(t.upload(c->d_mobj_fx));
        c->mfx_proto.steps = t.at<MfxStep>(steps);
        c->mfx_proto.chains = t.at<MfxChain>(chains);
        c->mfx_proto.types = t.at<MfxType>(types);
        c->mfx_proto.type_of = t.at<int32_t>(type_of);
        c->mfx_proto.events = t.at<MfxEvent>(events);
        c->mfx_proto.n_events = (uint32_t)mfx.events.size();
        c->mfx_proto.n_mobjs = (uint32_t)mfx.type_of.size();
    }
    TablePack t;
    const size_t segs = t.add(sc.fs_segs), leaf = t.add(sc.fs_seg_leaf), first = t.add(sc.fs_leaf_first), sectors = t.add(sc.fs_sectors);
    const size_t anims = t.add(sc.fs_anims), bitmaps = t.add(sc.fs_bitmaps), sky = t.add(sc.flat_sky), mobjs = t.add(sc.fs_mobjs);
    const size_t sframes = t.add(sc.sprite_frames), aoff = t.add(sc.fs_anc_off), anc = t.add(sc.fs_anc);
    const size_t wnodes = t.add(sc.walk_nodes), wleaf = t.add(sc.walk_leaf_sector);       // the pose kernels' descent (mobj_pose_core.h)
    const size_t flats = t.add(sc.fs_flats), seg_side = t.add(sc.fs_seg_side);             // what the flat rows start as; what the sidedef entries are searched by (§8p)
    const size_t heights = t.add(sc.fs_heights);                                         // what the sector height rows start as (view_rows_core.h)
    HIP_TRY(t.upload(c->d_fs_scene));
    FsParams &P = c->fs_proto;
    P = FsParams{};
    P.k = c->dk;
    P.segs = t.at<FsSeg>(segs); P.seg_leaf = t.at<uint16_t>(leaf); P.leaf_first = t.at<uint32_t>(first);
    P.sectors = t.at<FsSector>(sectors); P.anims = t.at<FsAnim>(anims);
    P.bitmaps = t.at<FsBitmap>(bitmaps); P.flat_sky = t.at<uint8_t>(sky);
    P.mobjs = t.at<FsMobj>(mobjs); P.sframes = t.at<FsSpriteFrame>(sframes);
    P.anc_off = t.at<uint32_t>(aoff); P.anc = t.at<FsAnc>(anc);
    P.n_segs = (uint32_t)sc.segs.size(); P.n_leaves = (uint32_t)sc.subsectors.size(); P.n_mobjs = (uint32_t)sc.mobjs.size();
    P.sprite_stride = fs_sprite_stride(P.n_mobjs);
    P.sbin_stride = fs_sbin_stride(P.sprite_stride, (size_t)c->cfg.width);
    const FsScratchLayout L = fs_scratch_layout((size_t)c->cfg.max_batch, P.n_segs);
    HIP_TRY(hip_alloc(c->d_fs_scratch, L.total));
    c->fs_zero_bytes = L.zero_bytes;
    c->fs_rows_dirty = true;
    uint8_t *const d = c->d_fs_scratch.get();
    P.occ = reinterpret_cast<uint32_t *>(d + L.occ);
    P.lite = reinterpret_cast<uint2 *>(d + L.lite);
    P.cl_rows = reinterpret_cast<uint32_t *>(d + L.cl_rows);
    P.keep_rows = reinterpret_cast<uint32_t *>(d + L.keep_rows);
    P.cl_row_cap = L.cl_row_cap;
    // the three kinds of per-view rows: the scene side of their kernels' arguments, and every slot's rows and entry staging, sized by
    // the scene like the scratch above (upload_view_rows).  The poses need map objects and a BSP, the other two sectors; the surfaces
    // bring their sidedef table, which stands or falls with the flats' buffers.
    const size_t n_sectors = sc.sectors.size();
    const bool pose_rows = P.n_mobjs && !sc.walk_nodes.empty();
    upload_view_rows(c, c->pose_proto, &Slot::PerScene::poses, pose_rows ? P.mobjs : nullptr, P.n_mobjs,
                     PoseCtx{t.at<WalkNode>(wnodes), t.at<int32_t>(wleaf), (int32_t)sc.walk_nodes.size() - 1});
    upload_view_rows(c, c->height_proto, &Slot::PerScene::heights, n_sectors ? t.at<FsHeights>(heights) : nullptr, n_sectors);
    upload_view_rows(c, c->flat_proto, &Slot::PerScene::flats, n_sectors ? t.at<FsFlats>(flats) : nullptr, n_sectors);
    c->d_seg_side = t.at<int32_t>(seg_side);
    const SurfaceLayout U = surface_layout((size_t)c->cfg.max_batch, n_sectors);
    for (Slot &s : c->slots) {
        Slot::PerScene &b = s.per_scene;
        if (!b.flats || hip_alloc(b.h_side_table, U.table) != hipSuccess || hip_alloc(b.d_side_table, U.table) != hipSuccess) {
            b.flats = {}; b.h_side_table.reset(); b.d_side_table.reset();
            (void)hipGetLastError();
        }
    }
    c->fs_scene_ok = true;
    return DG_OK;
}

// DG_FE_AUTO: should this batch's per-seg half run on the GPU?  The rule and what it has measured are fe_auto.hpp's; here: what is forced,
// the measuring, and what is in flight.  Small batches (< 64 frames: the kernels' fixed latency exceeds the host's few microseconds per
// frame) and prepared ones always go to the host walker.
void harvest_gpu_time(dg_ctx *c, Slot &s);
// First guess of the host walker's speed without spending a whole batch on it: a dozen of the batch's views on the calling thread
// (four untimed ones first), scaled by the pool size.  Whole batches that do go through the host walker refine it (build_batch_fe).
void calibrate_host(dg_ctx *c, const dg_view *views, int n) {
    const Scene &sc = *c->scene;
    FrameArena &A = *c->arenas[0];
    std::string err;
    const int warm = std::min(4, n), timed = std::min(8, n);
    for (int i = 0; i < warm; i++) { dg_view v = views[i]; fill_view_trig(v); (void)build_frame_parts(sc, c->cfg.width, c->cfg.height, v, A, err, {}, &c->fx); }
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < timed; i++) { dg_view v = views[n - 1 - i]; fill_view_trig(v); (void)build_frame_parts(sc, c->cfg.width, c->cfg.height, v, A, err, {}, &c->fx); }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->fe_auto.calibrated(ms, timed, c->n_threads);
}
bool choose_fs(dg_ctx *c, const dg_view *views, int n) {
    if (c->fs_forced) return true;
    if (n < 64 || c->preparing) return false;
    if (c->fe_auto.ema_host < 0.0) calibrate_host(c, views, n);
    bool in_flight = false;
    for (Slot &s : c->slots) { harvest_gpu_time(c, s); in_flight |= s.phase == Slot::Phase::Queued; }
    return c->fe_auto.seg_walk_next(in_flight);
}

// dg_light_rows / dg_mobj_rows complete the rows the seg walk reads (Rows: LfxRows / MfxRows, whose fields carry the same names).  R
// becomes the ctx's proto wired to one batch: `row` / `stride` as its base, `mask` the views' override masks (nullptr: no view states),
// `out` the rows it writes, n elements per frame.  The seg walk's `row` / `stride` move on to those.
template <class Rows, class T>
void wire_rows(Rows &R, const Rows &proto, const dg_view *views, int n_frames, const uint32_t *mask, T *out, size_t n, const T *&row, uint32_t &stride) {
    R = proto;
    R.views = views;
    R.n_frames = n_frames;
    R.base = row;
    R.base_stride = stride;
    R.mask = mask;
    R.mask_words = (uint32_t)((n + 31) / 32);
    R.out = out;
    row = out;
    stride = (uint32_t)n;
}

// One kind of per-view rows (view_rows_core.h) in a seg-walk batch.  Can the slot carry it for n frames — the scene has such rows, the
// slot got its buffers at dg_upload_scene, and the cells stay below the kernels' 2^31?  If not the batch takes the host walker, and
// is counted.
template <class K> bool carries_rows(dg_ctx *c, const RowBuffers<K> &b, const ViewRowParams<K> &proto, int n) {
    if (b && proto.scene_rows && K::ctx_ok(proto.ctx) && (uint64_t)n * proto.n_items < (1ull << 31)) return true;
    c->fallbacks_fe++;
    return false;
}
// This batch's arguments of the kind's kernels: n frames, the first n_entries of the slot's staging.
template <class K> void wire_view_rows(RowRun<K> &run, const ViewRowParams<K> &proto, const RowBuffers<K> &b, int n, uint32_t n_entries) {
    run.P = proto;
    run.P.entries = b.d_entries.get(); run.P.rows = b.rows.get();
    run.P.n_frames = (uint32_t)n; run.P.n_entries = n_entries;
}
// ... and their way to the device, on the slot's stream.
template <class K> hipError_t copy_row_entries(const RowBuffers<K> &b, uint32_t n_entries, hipStream_t stream) {
    if (!n_entries) return hipSuccess;
    return hipMemcpyAsync(b.d_entries.get(), b.h_entries.get(), (size_t)n_entries * sizeof(typename K::Entry), hipMemcpyHostToDevice, stream);
}

// DG_FE_DEVICE_SEGS: nothing of the front end runs on the host.  Per frame it ships the view (trig filled) and the DevFrame header,
// per batch the scene's current light levels and map-object states; dg_fs_* then write the same record arrays build_batch_fe packs,
// with fixed per-frame strides (fs_frame.h), into the slot's record slab.
int build_batch_fs(dg_ctx *c, Slot &s, const dg_view *views, int n, const BatchInputs &in) {
    const auto t0 = std::chrono::steady_clock::now();
    const dg_view_state *const states = in.states;
    const dg_view_poses *const poses = in.poses;
    const dg_view_sectors *const sectors = in.sectors;
    const dg_view_surfaces *const surfaces = in.surfaces;
    if (const int bad = check_batch(c, n)) return bad;
    const Scene &sc = *c->scene;
    const int W = c->cfg.width;
    const uint32_t span_stride = fe_span_stride(c);
    // per-view game state (dg_view_state): every frame gets its own copy of the two state arrays — the scene's values with the view's
    // entries on top — instead of one copy for the batch; the kernels index them with a per-frame stride
    const size_t state_frames = states ? (size_t)n : 1;
    // light effects (dg_light_rows): with view states, per frame a mask of the sectors its state overrides (the rows above are then
    // completed in place); without, the kernel writes the per-view rows from the one base row into the device-written part
    const bool lfx = c->lfx_proto.recs && c->fx.light.fits(sc);
    const size_t mask_words = (sc.sectors.size() + 31) / 32;
    // map-object thinkers (dg_mobj_rows): the same two layouts for the map-object rows
    const bool mfx = c->mfx_proto.steps && c->fx.mobj.fits(sc);
    if (mfx && (uint64_t)n * sc.mobjs.size() >= (1ull << 31)) return kPartsUnsupported;
    const size_t mmask_words = (sc.mobjs.size() + 31) / 32;
    const FsLayout L = fs_layout((size_t)n, (size_t)W, sc.sectors.size(), sc.mobjs.size(), states != nullptr, lfx, mfx, c->fs_proto.sprite_stride, c->fs_proto.sbin_stride);
    if (L.total > c->fe_slab_cap) return kPartsUnsupported;
    // per-view poses: the entries that stand, frame after frame, into the slot's staging; the pose kernels write the rows from them.
    // Without the slot's pose buffers (their allocation failed at dg_upload_scene) the batch takes the host walker, and is counted.
    uint32_t n_pose_entries = 0;
    const bool pose_rows = poses && !sc.mobjs.empty();
    if (poses && sc.mobjs.empty())                                    // (no entry can be valid)
        for (int i = 0; i < n; i++)
            if (poses[i].n) return set_err(DG_ERR_INVALID, "frame " + std::to_string(i) + ": view poses: map object index out of range");
    Slot::PerScene &B = s.per_scene;
    FrameArena &A = *c->arenas[0];
    if (pose_rows) {
        if (!carries_rows(c, B.poses, c->pose_proto, n)) return kPartsUnsupported;
        PoseEntry *const he = B.poses.h_entries.get();
        for (int i = 0; i < n; i++) {
            const bool ok = resolve_view_poses(sc, poses[i], A.poses);
            for (const dg_mobj_pose &p : A.poses.out) he[n_pose_entries++] = PoseEntry{i, p.mobj, p.x, p.y, p.angle};     // (at most one per object and frame: the staging holds them)
            A.poses.release();
            if (!ok) return set_err(DG_ERR_INVALID, "frame " + std::to_string(i) + ": view poses: map object index out of range");
        }
    }
    // per-view sector heights, likewise: the entries that stand into the slot's staging; the row kernels write the rows from them
    // (surfaces read heights through rows, with or without sector entries)
    uint32_t n_height_entries = 0;
    if ((sectors || surfaces) && !carries_rows(c, B.heights, c->height_proto, n)) return kPartsUnsupported;
    if (sectors) {
        SectorEntry *const he = B.heights.h_entries.get();
        for (int i = 0; i < n; i++) {
            const unsigned bad = resolve_view_sectors(sc, sectors[i], A.heights);
            for (const dg_sector_heights &e : A.heights.out) he[n_height_entries++] = SectorEntry{i, e.sector, (int16_t)e.floor_height, (int16_t)e.ceiling_height};   // (at most one per sector and frame: the staging holds them)
            A.heights.release();
            if (bad) return set_err(DG_ERR_INVALID, "frame " + std::to_string(i) + ": " + view_sectors_error(bad));
        }
    }
    // per-view surfaces, likewise: the flat entries that stand into the slot's staging, and the sidedef entries frame after frame,
    // sorted, behind their offsets first[frame].  More sidedef entries than the table holds: the host walker, counted.
    uint32_t n_flat_entries = 0, n_side_entries = 0;
    const SurfaceLayout U = surface_layout((size_t)c->cfg.max_batch, sc.sectors.size());
    if (surfaces) {
        if (!carries_rows(c, B.flats, c->flat_proto, n)) return kPartsUnsupported;
        FlatEntry *const fe = B.flats.h_entries.get();
        uint32_t *const first = reinterpret_cast<uint32_t *>(B.h_side_table.get());
        FsSideEntry *const se = reinterpret_cast<FsSideEntry *>(B.h_side_table.get() + U.first_bytes);
        for (int i = 0; i < n; i++) {
            const unsigned bad = resolve_view_surfaces(sc, c->fx.wall.on() ? &c->fx.wall : nullptr, surfaces[i], i, A.sides, A.flats);
            if (bad) return set_err(DG_ERR_INVALID, "frame " + std::to_string(i) + ": " + view_surfaces_error(bad));
            if ((size_t)n_side_entries + A.sides.out.size() > U.side_cap) { c->fallbacks_fe++; return kPartsUnsupported; }
            first[i] = n_side_entries;
            for (const FsSideEntry &e : A.sides.out) se[n_side_entries++] = e;
            for (const FlatEntry &e : A.flats.out) fe[n_flat_entries++] = e;                               // (at most one per sector and frame: the staging holds them)
        }
        first[n] = n_side_entries;
    }
    uint8_t *const h = s.h_fe.get(), *const d = s.d_fe.get();
    s.views.assign(views, views + n);
    c->pool->parallel_for(n, [&](int i, int) {
        dg_view &v = s.views[(size_t)i];
        fill_view_trig(v);
        DevFrame hdr = make_frame_header(v);
        hdr.span_base = (uint32_t)i * span_stride;
        std::memcpy(h + L.frames + (size_t)i * sizeof(DevFrame), &hdr, sizeof hdr);
        std::memcpy(h + L.views + (size_t)i * sizeof(dg_view), &v, sizeof v);
    });
    int16_t *lights = reinterpret_cast<int16_t *>(h + L.lights);
    int32_t *mstate = reinterpret_cast<int32_t *>(h + L.mstate);
    uint32_t *lmask = reinterpret_cast<uint32_t *>(h + L.lmask);
    uint32_t *mmask = reinterpret_cast<uint32_t *>(h + L.mmask);
    std::atomic<int> bad_state{-1};
    c->pool->parallel_for((int)state_frames, [&](int i, int) {
        int16_t *l = lights + (size_t)i * sc.sectors.size();
        int32_t *m = mstate + (size_t)i * sc.mobjs.size();
        for (size_t k = 0; k < sc.sectors.size(); k++) l[k] = sc.sectors[k].light;
        for (size_t k = 0; k < sc.mobjs.size(); k++) m[k] = mfx_encode(sc.mobjs[k].sprite_frame, sc.mobjs[k].full_bright);
        if (!states) return;
        uint32_t *lm = lfx ? lmask + (size_t)i * mask_words : nullptr;
        if (lm) std::memset(lm, 0, mask_words * 4);
        uint32_t *mm = mfx ? mmask + (size_t)i * mmask_words : nullptr;
        if (mm) std::memset(mm, 0, mmask_words * 4);
        const unsigned bad = apply_view_state(
            sc, states[i],
            [&](size_t k, int32_t level) { l[k] = (int16_t)level; if (lm) lm[k / 32] |= 1u << (k % 32); },
            [&](size_t k, int32_t val) { m[k] = val; if (mm) mm[k / 32] |= 1u << (k % 32); });
        if (bad) bad_state = i;
    });
    if (bad_state >= 0) return set_err(DG_ERR_INVALID, "frame " + std::to_string(bad_state.load()) + ": view state: sector, map object or sprite frame index out of range");

    FsParams &Q = s.FSP;
    Q = c->fs_proto;
    Q.sector_light = reinterpret_cast<const int16_t *>(d + L.lights);
    Q.mobj_state = reinterpret_cast<const int32_t *>(d + L.mstate);
    Q.light_stride = states ? (uint32_t)sc.sectors.size() : 0u;
    Q.mstate_stride = states ? (uint32_t)sc.mobjs.size() : 0u;
    Q.views = reinterpret_cast<const dg_view *>(d + L.views);
    Q.n_frames = n;
    s.pose_run.P = {}; s.height_run.P = {}; s.flat_run.P = {}; s.SF = FsSurf{};
    if (pose_rows) {                                       // the seg walk reads the rows dg_mobj_pose_fill / _place write
        wire_view_rows(s.pose_run, c->pose_proto, B.poses, n, n_pose_entries);
        Q.mobjs = s.pose_run.P.rows; Q.mobj_stride = s.pose_run.P.n_items;
    }
    if (sectors || surfaces) wire_view_rows(s.height_run, c->height_proto, B.heights, n, n_height_entries);   // the row-reading seg walk reads the rows dg_sector_row_fill / _scatter write
    if (surfaces) {                                        // the dg_sfc_* pair reads both kinds of rows and the sidedef table
        wire_view_rows(s.flat_run, c->flat_proto, B.flats, n, n_flat_entries);
        const uint8_t *const dt = B.d_side_table.get();
        s.SF = FsSurf{s.height_run.P.rows, s.flat_run.P.rows, s.flat_run.P.n_items, reinterpret_cast<const FsSideEntry *>(dt + U.first_bytes), reinterpret_cast<const uint32_t *>(dt), c->d_seg_side};
    }
    s.LR = LfxRows{};
    if (lfx) wire_rows(s.LR, c->lfx_proto, Q.views, n, states ? reinterpret_cast<const uint32_t *>(d + L.lmask) : nullptr,
                       reinterpret_cast<int16_t *>(d + (states ? L.lights : L.lrows)), sc.sectors.size(), Q.sector_light, Q.light_stride);
    s.MR = MfxRows{};
    if (mfx) wire_rows(s.MR, c->mfx_proto, Q.views, n, states ? reinterpret_cast<const uint32_t *>(d + L.mmask) : nullptr,
                       reinterpret_cast<int32_t *>(d + (states ? L.mstate : L.mrows)), sc.mobjs.size(), Q.mobj_state, Q.mstate_stride);
    Q.flags = s.d_flags.get();
    point_at_records(Q, d, L);                             // the seg walk writes what the column walk reads
    FeParams &F = s.FP;
    point_at(F.frames, d, L.frames);
    point_at_records(F, d, L);
    F.max_sky_slots = FS_SKY_CAP; F.gap_waves = 12;
    Q.order_cnt = s.d_flags.get() + c->cfg.max_batch;      // zeroed with the flags (enqueue_kernels)
    Q.order_list = s.d_order.get();
    Q.n_items = (uint32_t)n * (uint32_t)fe_col_groups((size_t)W);
    F.order = Q.order_list; F.order_cnt = Q.order_cnt;
    fill_walk_params(c, s, n);
    s.describe(DG_FE_DEVICE_SEGS, n, L.upload, 0, 0);
    s.snapshot_scene(sc);
    s.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(hipMemcpyAsync(d, h, L.upload, hipMemcpyHostToDevice, s.stream.get()));
    HIP_TRY(copy_row_entries(B.poses, n_pose_entries, s.stream.get()));
    HIP_TRY(copy_row_entries(B.heights, n_height_entries, s.stream.get()));
    HIP_TRY(copy_row_entries(B.flats, n_flat_entries, s.stream.get()));
    if (surfaces) HIP_TRY(hipMemcpyAsync(B.d_side_table.get(), B.h_side_table.get(), U.first_bytes + (size_t)n_side_entries * sizeof(FsSideEntry), hipMemcpyHostToDevice, s.stream.get()));
    return DG_OK;
}

int build_batch(dg_ctx *c, Slot &s, const dg_view *views, const dg_frame_lists *given, int n, const BatchInputs &in) {
    if (!given && c->fs_enabled && c->fs_scene_ok && choose_fs(c, views, n)) {
        const int rc = build_batch_fs(c, s, views, n, in);
        if (rc != kPartsUnsupported) return rc;
    }
    if (!given && c->fe_enabled && c->fe_scene_ok) {
        const int rc = build_batch_fe(c, s, views, n, in);
        if (rc != kPartsUnsupported) return rc;
    }
    return build_batch_host(c, s, views, given, n, in);
}

// The 2-D map view's linedef layer of the uploaded scene, on the kernel stream (timed by the slot's ev_start / ev_setup).  The line records
// and the W*H owner words are transient: freed once the layer is built.
int build_map_layer(dg_ctx *c, Slot &s) {
    const int W = c->cfg.width, H = c->cfg.height;
    std::vector<dg_map_line> lines;
    std::string err;
    int rc = map_frame_lines(*c->scene, W, H, nullptr, lines, err);
    if (rc) return set_err(rc, err);
    const size_t n = lines.size();
    std::vector<MapSeg> segs(std::max<size_t>(n, 1));
    std::vector<uint32_t> base(n + 1);
    uint64_t total = 0;
    for (size_t k = 0; k < n; k++) {
        const dg_map_line &l = lines[k];
        segs[k] = map_seg_make(l.x0, l.y0, l.x1, l.y1, l.rgb, W, H);
        base[k] = (uint32_t)total;
        total += (uint64_t)segs[k].count;
    }
    if (total >= (1ull << 31)) return set_err(DG_ERR_CAPACITY, "map layer: too many line steps");
    base[n] = (uint32_t)total;
    DevPtr<uint8_t> layer, tmp;
    HIP_TRY(hip_alloc(layer, (size_t)3 * (size_t)W * (size_t)H));
    SlabCursor cur;
    const size_t off_owner = cur.take((size_t)W * (size_t)H * 4), off_segs = cur.take(segs.size() * sizeof(MapSeg)), off_base = cur.take(base.size() * 4);
    HIP_TRY(hip_alloc(tmp, cur.end()));
    uint32_t *owner = reinterpret_cast<uint32_t *>(tmp.get() + off_owner);
    MapSeg *d_segs = reinterpret_cast<MapSeg *>(tmp.get() + off_segs);
    uint32_t *d_base = reinterpret_cast<uint32_t *>(tmp.get() + off_base);
    HIP_TRY(hipMemcpy(d_segs, segs.data(), segs.size() * sizeof(MapSeg), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_base, base.data(), base.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(owner, 0, (size_t)W * (size_t)H * 4, c->kstream.get()));
    HIP_TRY(launch_map_layer(d_segs, d_base, (uint32_t)n, (uint32_t)total, owner, layer.get(), W, H, c->kstream.get(), s.ev_start.get(), s.ev_setup.get()));
    HIP_TRY(hipStreamSynchronize(c->kstream.get()));           // (before the transient buffers go)
    c->per_scene.map_layer = std::move(layer);
    return DG_OK;
}

// Host tables into device memory on the kernel stream, between the slot's ev_start / ev_setup; done when it returns (the host copies may go).
struct TableCopy { void *dst; const void *src; size_t bytes; };
int upload_timed(dg_ctx *c, Slot &s, const TableCopy *copies, size_t n) {
    HIP_TRY(hipEventRecord(s.ev_start.get(), c->kstream.get()));
    for (size_t k = 0; k < n; k++)
        if (copies[k].bytes) HIP_TRY(hipMemcpyAsync(copies[k].dst, copies[k].src, copies[k].bytes, hipMemcpyHostToDevice, c->kstream.get()));
    HIP_TRY(hipEventRecord(s.ev_setup.get(), c->kstream.get()));
    HIP_TRY(hipStreamSynchronize(c->kstream.get()));
    return DG_OK;
}
int upload_timed(dg_ctx *c, Slot &s, std::initializer_list<TableCopy> copies) { return upload_timed(c, s, copies.begin(), copies.size()); }

// The explored-map frames' cover of the uploaded scene at the ctx's frame size, built on the host (explored_cover.hpp).
int upload_explored_cover(dg_ctx *c, Slot &s) {
    ExploredCover cv;
    std::string err;
    const int rc = build_explored_cover(*c->scene, c->cfg.width, c->cfg.height, cv, err);
    if (rc) return set_err(rc, err);
    DevPtr<uint32_t> cover, chains;
    HIP_TRY(hip_alloc(cover, cv.cover.size() * 4));
    HIP_TRY(hip_alloc(chains, cv.chains.size() * 4));
    if (const int bad = upload_timed(c, s, {{cover.get(), cv.cover.data(), cv.cover.size() * 4}, {chains.get(), cv.chains.data(), cv.chains.size() * 4}})) return bad;
    c->per_scene.chains = std::move(chains);
    c->per_scene.cover = std::move(cover);
    return DG_OK;
}

// The player-centred map frames' line table of the uploaded scene (ego_line_table).
int upload_ego_table(dg_ctx *c, Slot &s) {
    std::vector<EgoLine> lines;
    std::vector<uint32_t> words;
    ego_line_table(*c->scene, lines, words);
    const size_t L = lines.size();
    DevPtr<uint8_t> table;
    HIP_TRY(hip_alloc(table, L * (sizeof(EgoLine) + sizeof(uint32_t))));
    if (const int bad = upload_timed(c, s, {{table.get(), lines.data(), L * sizeof(EgoLine)}, {table.get() + L * sizeof(EgoLine), words.data(), L * sizeof(uint32_t)}})) return bad;
    c->per_scene.ego_lines = (uint32_t)L;
    c->per_scene.ego_table = std::move(table);
    return DG_OK;
}

// The floor-textured map frames' tables of the uploaded scene (floor_tables) in one allocation — and, in the same timed upload, the
// player-centred frames' line table when no submission has made it yet: dg_floor_map_tiles reads both.
int upload_floor_table(dg_ctx *c, Slot &s) {
    const Scene &sc = *c->scene;
    FloorHostTables t;
    floor_tables(sc, t);
    SlabCursor cur;
    const size_t at_segs = cur.take(t.segs.size() * sizeof(FloorSeg)), at_nodes = cur.take(sc.walk_nodes.size() * sizeof(WalkNode));
    const size_t at_leaves = cur.take(t.leaves.size() * sizeof(FloorLeaf)), at_lines = cur.take(t.lines.size() * sizeof(FloorLine));
    DevPtr<uint8_t> table, ego;
    HIP_TRY(hip_alloc(table, std::max<size_t>(cur.end(), 16)));
    uint8_t *const d = table.get();
    std::vector<TableCopy> copies{{d + at_segs, t.segs.data(), t.segs.size() * sizeof(FloorSeg)}, {d + at_nodes, sc.walk_nodes.data(), sc.walk_nodes.size() * sizeof(WalkNode)},
                                  {d + at_leaves, t.leaves.data(), t.leaves.size() * sizeof(FloorLeaf)}, {d + at_lines, t.lines.data(), t.lines.size() * sizeof(FloorLine)}};
    std::vector<EgoLine> lines;
    std::vector<uint32_t> words;
    const bool with_ego = !c->per_scene.ego_table;
    if (with_ego) {
        ego_line_table(sc, lines, words);
        const size_t L = lines.size();
        HIP_TRY(hip_alloc(ego, L * (sizeof(EgoLine) + sizeof(uint32_t))));
        copies.push_back({ego.get(), lines.data(), L * sizeof(EgoLine)});
        copies.push_back({ego.get() + L * sizeof(EgoLine), words.data(), L * sizeof(uint32_t)});
    }
    if (const int bad = upload_timed(c, s, copies.data(), copies.size())) return bad;
    dg_ctx::PerScene &p = c->per_scene;
    if (with_ego) { p.ego_lines = (uint32_t)lines.size(); p.ego_table = std::move(ego); }
    p.floor_T = FloorTables{reinterpret_cast<const WalkNode *>(d + at_nodes), (uint32_t)sc.walk_nodes.size(), reinterpret_cast<const FloorLeaf *>(d + at_leaves),
                            (uint32_t)t.leaves.size(), reinterpret_cast<const FloorSeg *>(d + at_segs), (uint32_t)t.segs.size(), c->d_flats,
                            (uint32_t)(c->uploaded_flats / 4096u), c->d_palette.get(), (uint32_t)sc.sectors.size()};
    p.floor_lines = reinterpret_cast<const FloorLine *>(d + at_lines);
    p.floor_table = std::move(table);
    return DG_OK;
}

// The marker and place tables of the uploaded scene (thing_tables) with the marker table the ctx took, for the map frames with markers:
// one allocation, made by the first such submission after dg_upload_scene (untimed: 28 bytes per map object).  No marker table: an
// empty one, and the kernels' things phase has nothing to do.
int upload_thing_table(dg_ctx *c) {
    const Scene &sc = *c->scene;
    const std::vector<dg_map_marker> *markers = thing_markers(sc, c->markers);
    std::vector<ThingMarker> tm;
    std::vector<ThingPlace> tp;
    if (markers) thing_tables(sc, *markers, tm, tp);
    const size_t n = tm.size();
    DevPtr<uint8_t> table;
    HIP_TRY(hip_alloc(table, std::max<size_t>(n * (sizeof(ThingMarker) + sizeof(ThingPlace)), 16)));
    if (n) {
        HIP_TRY(hipMemcpyAsync(table.get(), tp.data(), n * sizeof(ThingPlace), hipMemcpyHostToDevice, c->kstream.get()));
        HIP_TRY(hipMemcpyAsync(table.get() + n * sizeof(ThingPlace), tm.data(), n * sizeof(ThingMarker), hipMemcpyHostToDevice, c->kstream.get()));
        HIP_TRY(hipStreamSynchronize(c->kstream.get()));  // (before the host copies go)
    }
    c->per_scene.things = (uint32_t)n;
    c->per_scene.thing_table = std::move(table);
    return DG_OK;
}

// The per-scene table of the slot's map kind: built by the first such submission after dg_upload_scene, which then has a timed front half.
int ensure_map_table(dg_ctx *c, Slot &s) {
    s.map.built = false;
    int rc;
    switch (s.front_end) {
    case DG_FE_MAP: if (c->per_scene.map_layer) return DG_OK; rc = build_map_layer(c, s); break;
    case DG_FE_MAP_EXPLORED: if (c->per_scene.cover) return DG_OK; rc = upload_explored_cover(c, s); break;
    case DG_FE_MAP_FLOOR: if (c->per_scene.floor_table) return DG_OK; rc = upload_floor_table(c, s); break;
    default: if (c->per_scene.ego_table) return DG_OK; rc = upload_ego_table(c, s); break;
    }
    s.map.built = rc == DG_OK;
    return rc;
}

// Where a map submission of n frames keeps what follows its arrow lines in the slot's list slab: a player-centred submission's views.
size_t ego_views_at(int n) { return (size_t)n * 3 * sizeof(MapSeg); }

constexpr size_t kOverlapMaxPixels = 500000;          // frames up to this size overlap their raster launch with the next batch's front end (dg_create)

// A submission's last step: its kernels are enqueued.  harvested: DG_FE_AUTO has nothing to read from it.
int queued(Slot &s, bool harvested = true) {
    s.harvested = harvested;
    s.raster_recorded = true;
    s.phase = Slot::Phase::Queued;
    return DG_OK;
}

// The slot's kernels go on stream ks behind its upload, which is queued on the slot's own stream.
int after_upload(Slot &s, hipStream_t ks) {
    HIP_TRY(hipEventRecord(s.ev_h2d.get(), s.stream.get()));
    HIP_TRY(hipStreamWaitEvent(ks, s.ev_h2d.get(), 0));
    return DG_OK;
}

// A launch that fails leaves the slot empty: later calls on it return DG_ERR_INVALID instead of reading what nobody wrote.
struct Invalidate {
    Slot &s; bool armed = true;
    ~Invalidate() { if (armed) s.reset(); }
};

// The kernels of the map submission the slot describes, on the ctx's kernel stream behind its upload: the kind's per-scene table if it
// is not there yet, then the kind's frame kernels.  A HIP call that fails half way leaves the slot empty.
int enqueue_map_frames(dg_ctx *c, Slot &s) {
    hipStream_t ks = c->kstream.get();
    Invalidate guard{s};
    if (const int rc = after_upload(s, ks)) return rc;
    if (const int rc = ensure_map_table(c, s)) return rc;
    const dg_ctx::PerScene &t = c->per_scene;
    const MapSeg *const arrow = reinterpret_cast<const MapSeg *>(s.d_lists.get());
    const int W = c->cfg.width, H = c->cfg.height;
    if (s.front_end == DG_FE_MAP) {                       // the layer copied + the arrow, per frame
        HIP_TRY(launch_map_frames(t.map_layer.get(), arrow, s.n_frames, s.d_fb.get(), W, H, ks, s.ev_rstart.get(), s.ev_raster.get()));
    } else if (s.front_end == DG_FE_MAP_EXPLORED) {       // the cover picked through the frame's mask row + the arrow, per frame
        HIP_TRY(launch_explored_frames(t.cover.get(), t.chains.get(), s.per_scene.d_masks.get(), (uint32_t)s.per_scene.mask_words, arrow, s.n_frames, s.d_fb.get(),
                                       W, H, ks, s.ev_rstart.get(), s.ev_raster.get()));
    } else {                                              // player-centred: one kernel; floor-textured: the mask's sector rows, then one kernel
        EgoParams E{};
        E.lines = reinterpret_cast<const EgoLine *>(t.ego_table.get());
        E.words = reinterpret_cast<const uint32_t *>(t.ego_table.get() + (size_t)t.ego_lines * sizeof(EgoLine));
        E.n_lines = t.ego_lines;
        E.views = reinterpret_cast<const EgoView *>(s.d_lists.get() + ego_views_at(s.n_frames));
        E.arrow = (s.map.ego.flags & EGO_ARROW) ? arrow : nullptr;
        E.masks = s.map.masked ? s.per_scene.d_masks.get() : nullptr;
        E.mask_words = (uint32_t)s.per_scene.mask_words;
        E.scale = s.map.ego.scale; E.rotate = s.map.ego.flags & EGO_ROTATE;
        E.W = W; E.H = H;
        E.fb = s.d_fb.get(); E.n_frames = s.n_frames;
        ThingParams T{};                                  // a *_things submission: the same frames through the kernels with the things phase
        if (s.map.things) {
            if (!t.thing_table) { if (const int rc = upload_thing_table(c)) return rc; }
            const uint8_t *const d = s.per_scene.d_things.get();
            T.places = reinterpret_cast<const ThingPlace *>(t.thing_table.get());
            T.markers = reinterpret_cast<const ThingMarker *>(t.thing_table.get() + (size_t)t.things * sizeof(ThingPlace));
            T.n_things = t.things;
            T.shown = reinterpret_cast<const uint32_t *>(d);
            T.shown_words = thing_shown_words(t.things);
            T.first = reinterpret_cast<const uint32_t *>(d + s.map.things_first);
            T.entries = reinterpret_cast<const ThingEntry *>(d + s.map.things_entries);
        }
        if (s.front_end == DG_FE_MAP_FLOOR) {
            const Slot::PerScene &b = s.per_scene;
            const uint32_t seen_words = (uint32_t)floor_seen_words(*c->scene);
            if (E.masks) HIP_TRY(launch_floor_seen_sectors(t.floor_lines, t.ego_lines, t.floor_T.n_sectors, E.masks, E.mask_words, b.d_floor_seen.get(), seen_words, s.n_frames, ks));
            const FloorMapParams Q{E, t.floor_T, b.d_floor_cells.get(), E.masks ? b.d_floor_seen.get() : nullptr, seen_words, 1.0f / s.map.ego.scale};
            if (s.map.things) HIP_TRY(launch_floor_thing_tiles(Q, T, ks, s.ev_rstart.get(), s.ev_raster.get()));
            else HIP_TRY(launch_floor_map_tiles(Q, ks, s.ev_rstart.get(), s.ev_raster.get()));
        } else if (s.map.things) HIP_TRY(launch_ego_thing_tiles(E, T, ks, s.ev_rstart.get(), s.ev_raster.get()));
        else HIP_TRY(launch_ego_tiles(E, ks, s.ev_rstart.get(), s.ev_raster.get()));
    }
    guard.armed = false;
    return queued(s);                                     // (never DG_FE_AUTO's measurement)
}

int enqueue_kernels(dg_ctx *c, Slot &s) {
    if (s.map_frames()) return enqueue_map_frames(c, s);
    // All kernels of all slots run on ONE in-order stream (highest priority, so that it gets a hardware queue of its own): column walk
    // i, rasteriser i, column walk i + 1, ...  The slot's own stream carries its H2D copy (queued already; it overlaps the previous
    // slots' kernels), tied in with an event.  Letting the walk of batch i + 1 overlap the raster launch of batch i was measured to buy
    // nothing at 1280x800: its waves take slots a raster workgroup needs as a whole, the launch stretches by what the walk costs alone
    // (profiles/r03_column_walk.md) — for small frames it does pay, and the raster launches then go to a second stream (raster_overlap).  The walk's per-frame status words (overflow flags, span totals) live in pinned host memory and are
    // written by the kernels directly: nothing is queued behind the raster launch, so no stream ever holds a barrier that another
    // slot's upload could get stuck behind (streams share hardware queues).
    hipStream_t ks = c->kstream.get();
    Invalidate guard{s};                                  // (a HIP call that fails half way: nobody wrote the status words)
    const bool fe_mode = s.column_walk();
    if (const int rc = after_upload(s, ks)) return rc;
    if (fe_mode) {
        std::memset(s.h_status.get(), 0, (size_t)2 * (size_t)c->cfg.max_batch * 4);
        // the overflow flags, the launch-order counters and the event bits behind them start from zero: dg_fe_scan leaves them so (its
        // last lines), and only a slot that is new or whose last enqueue failed half way is cleared here, whole
        if (!s.walk_state_clean) HIP_TRY(hipMemsetAsync(s.d_flags.get(), 0, s.walk_state_bytes, ks));
        s.walk_state_clean = false;
        if (s.seg_walk()) {                                                                             // the seg walk writes what the column walk reads
            if (c->fs_rows_dirty) HIP_TRY(hipMemsetAsync(c->d_fs_scratch.get(), 0, c->fs_zero_bytes, ks));    // (dg_fs_frame leaves its rows clean)
            c->fs_rows_dirty = true;
            // The batch's start event goes to whichever launch comes first; every later one takes its own, if it has one.
            hipEvent_t first = s.ev_start.get();
            const auto start = [&first](hipEvent_t own) { const hipEvent_t e = first ? first : own; first = nullptr; return e; };
            const auto rows = [&](auto &run) {                                 // one kind of per-view rows, when the batch carries it
                if (!run.on()) return hipSuccess;
                run.from_start = first != nullptr;
                return launch_view_rows(run.P, ks, start(run.t0.get()), run.t1.get());
            };
            HIP_TRY(rows(s.pose_run));                                                                    // the rows dg_fs_frame's map-object phase reads
            if (s.LR.n_frames > 0) HIP_TRY(launch_light_rows(s.LR, ks, start(nullptr)));                   // the rows dg_fs_* read
            if (s.MR.n_frames > 0) HIP_TRY(launch_mobj_rows(s.MR, ks, start(nullptr)));
            HIP_TRY(rows(s.height_run));
            HIP_TRY(rows(s.flat_run));
            const bool wfx = c->fx.wall.on();
            const FsRows R{s.height_run.P.rows, s.height_run.P.n_items};
            if (s.flat_run.on()) {                          // the pair that reads the height rows, the flat rows and the sidedef table
                HIP_TRY(wfx ? launch_fs_surf_fx(s.FSP, FsSurfFx{c->fs_fx, s.SF}, ks, start(nullptr)) : launch_fs_surf(s.FSP, s.SF, ks, start(nullptr)));
            } else if (s.height_run.on()) {                 // the pair that reads the height rows
                HIP_TRY(wfx ? launch_fs_rows_fx(s.FSP, FsRowsFx{c->fs_fx, R.rows, R.stride}, ks, start(nullptr)) : launch_fs_rows(s.FSP, R, ks, start(nullptr)));
            } else {
                HIP_TRY(wfx ? launch_fs_fx(s.FSP, c->fs_fx, ks, start(nullptr)) : launch_fs(s.FSP, ks, start(nullptr)));
            }
            c->fs_rows_dirty = false;
        }
        HIP_TRY(launch_fe(s.FP, ks, s.seg_walk() ? nullptr : s.ev_start.get(), s.ev_setup.get()));
    } else {
        HIP_TRY(launch_setup(s.P, s.max_spans, ks, s.ev_start.get(), s.ev_setup.get()));
    }
    if (c->raster_overlap && fe_mode) {                   // the front end of the next batch may start while this launch runs (the column scratch is the front end's alone)
        HIP_TRY(hipStreamWaitEvent(c->rstream.get(), s.ev_setup.get(), 0));
        HIP_TRY(launch_raster(s.P, c->rstream.get(), s.ev_rstart.get(), s.ev_raster.get()));
    } else {
        HIP_TRY(launch_raster(s.P, ks, s.ev_rstart.get(), s.ev_raster.get()));
    }
    if (fe_mode) s.walk_state_clean = true;               // everything was enqueued: dg_fe_scan will have cleaned up by the slot's next batch
    guard.armed = false;
    return queued(s, !fe_mode);                           // (only a column-walk batch is DG_FE_AUTO's measurement)
}

// One frame of a device-column-walk batch again, through the host list path, into its place in the slot's framebuffer.  The
// slot's own prepared state (records, column index, resolved spans of the other frames) is not touched: the host list slab of
// the slot, unused in device mode, carries the one frame, its resolved spans go to a ctx-wide scratch.  Returns DG_ERR_CAPACITY
// when the frame does not fit that scratch (the caller then redoes the whole batch).
int redo_frame_host(dg_ctx *c, Slot &s, int i) {
    const Scene &sc = *c->scene;
    const int W = c->cfg.width, H = c->cfg.height;
    BinnedFrame &bf = c->binned[0];
    std::string err;
    dg_view v = s.views[(size_t)i];
    fill_view_trig(v);
    dg_frame_lists fl;
    Slot::RedoState redo_state;
    ViewInputs in = s.kept.at(i);
    in.state = s.state_for_redo(sc, i, redo_state, c->fx);
    int rc = build_frame_lists(sc, W, H, v, *c->arenas[0], fl, err, in, &c->fx);
    if (!rc) rc = bin_frame(sc, c->fk, fl, bf, err);
    if (rc) return set_err(rc, "frame " + std::to_string(i) + ": " + err);
    bf.hdr.span_base = 0; bf.hdr.wall_base = 0; bf.hdr.plane_base = 0;
    const ListLayout L = list_layout(1, (size_t)W, bf.walls.size(), bf.planes.size(), bf.spans.size());
    if (L.total > s.lists_cap) return DG_ERR_CAPACITY;
    if (!c->d_redo_rspans) {
        c->redo_span_cap = (size_t)W * 64;                                   // 64 spans per column on average: far beyond any real frame
        if (hip_alloc(c->d_redo_rspans, c->redo_span_cap * sizeof(DevRSpan)) != hipSuccess) return DG_ERR_CAPACITY;
    }
    if (bf.spans.size() > c->redo_span_cap) return DG_ERR_CAPACITY;
    pack_binned(s.h_lists.get(), L, bf, 0, (size_t)W);
    HIP_TRY(hipMemcpyAsync(s.d_lists.get(), s.h_lists.get(), L.total, hipMemcpyHostToDevice, s.stream.get()));
    RasterParams Q = s.P;
    point_at_lists(Q, s.d_lists.get(), L);
    Q.rspans = c->d_redo_rspans.get();
    Q.fb = s.d_fb.get() + (size_t)i * (size_t)3 * (size_t)W * (size_t)H;
    Q.n_frames = 1;
    HIP_TRY(launch_setup(Q, (uint32_t)bf.spans.size(), s.stream.get()));
    HIP_TRY(launch_raster(Q, s.stream.get()));
    HIP_TRY(slot_sync(s));                                 // the host slab is reused by the next frame
    return DG_OK;
}

// The overflow flags of a column-walk submission whose kernels have finished (make_final): a batch that overflowed a per-column /
// per-frame capacity is redone through the host list path (which has the larger limits).
int redo_overflowed(dg_ctx *c, Slot &s) {
    const uint32_t *const status = s.h_status.get();      // [max_batch] overflow flags, [max_batch] spans per frame
    bool overflow = false;
    uint64_t spans = 0;
    for (int i = 0; i < s.n_frames; i++) {
        overflow |= status[i] != 0;
        spans += status[c->cfg.max_batch + i];
    }
    s.n_spans = spans;
    if (!overflow) return DG_OK;
    // Only the frames that overflowed are redone (through the host list path, one at a time); if one of them does not fit the
    // single-frame scratch either, the whole batch is.
    c->fallbacks_fe++;
    bool whole_batch = false;
    for (int i = 0; i < s.n_frames && !whole_batch; i++) {
        if (status[i] == 0) continue;
        const int rc = redo_frame_host(c, s, i);
        if (rc == DG_ERR_CAPACITY) whole_batch = true;
        else if (rc) return rc;
        else c->redone_frames++;
    }
    if (!whole_batch) return DG_OK;
    // (the whole batch again, with every frame's submit-time state and the slot's own kept inputs: build_batch_host reads them while it
    // runs and, like every builder, writes nothing to s.kept — built_from, which does, is not called here)
    const std::vector<dg_view> views = s.views;
    std::vector<Slot::RedoState> redo_states(views.size());
    std::vector<dg_view_state> sts;
    bool any_state = false;
    for (size_t i = 0; i < views.size(); i++) {
        const dg_view_state *st = s.state_for_redo(*c->scene, (int)i, redo_states[i], c->fx);
        any_state |= st != nullptr;
        sts.push_back(st ? *st : dg_view_state{nullptr, 0, nullptr, 0});
    }
    BatchInputs in = s.kept.inputs();
    in.states = any_state ? sts.data() : nullptr;
    int rc = build_batch_host(c, s, views.data(), nullptr, (int)views.size(), in);
    if (rc) return rc;
    rc = enqueue_kernels(c, s);
    if (rc) return rc;
    return make_final(c, s, Copy::Leave);                  // (a host-list batch now: it is waited for, there are no flags to look at)
}

// DG_FE_AUTO's measurement of the GPU side: the span of a finished submission's kernels (never waits)
void harvest_gpu_time(dg_ctx *c, Slot &s) {
    if (s.harvested || !s.has_run() || !s.column_walk() || s.n_frames < 64 || c->fs_forced || !c->fs_enabled) return;
    if (hipEventQuery(s.ev_raster.get()) != hipSuccess) return;
    s.harvested = true;
    float ms = 0.0f;
    if (c->raster_overlap) {                               // the raster launch may have waited behind the previous batch's: the two halves' own durations
        float fe_ms = 0.0f, r_ms = 0.0f;
        if (hipEventElapsedTime(&fe_ms, s.ev_start.get(), s.ev_setup.get()) != hipSuccess || hipEventElapsedTime(&r_ms, s.ev_rstart.get(), s.ev_raster.get()) != hipSuccess) return;
        ms = std::max(fe_ms, r_ms);                        // (they overlap with the neighbouring batches': the longer one sets the pace)
        if (!(ms > 0.0f)) return;
    } else if (hipEventElapsedTime(&ms, s.ev_start.get(), s.ev_raster.get()) != hipSuccess || !(ms > 0.0f)) return;
    c->fe_auto.gpu_batch(s.seg_walk(), (double)ms, s.n_frames);
}

}  // namespace

// Making the last submission's results final, the one way from queued to settled: everything queued for the slot has finished, and the
// overflow flags of a column-walk batch are looked at, once per enqueue (frames that overflowed are redone here).  On a slot that is
// not queued this only waits, for a prepared slot's upload.  Copy::Complete is the wait path (dg_wait, take_slot): it owns the slot's
// pending asynchronous readback as well — completed, and issued again after a redo, because its first copy took frames of the overflowed
// run — and it is where DG_FE_AUTO reads the batch's GPU time.  Copy::Leave leaves both alone.
int dg::make_final(dg_ctx *c, Slot &s, Copy copy) {
    HIP_TRY(slot_sync(s));
    if (copy == Copy::Complete) harvest_gpu_time(c, s);
    const uint64_t redone = c->fallbacks_fe;
    const bool check = s.unchecked();
    if (s.phase == Slot::Phase::Queued) s.phase = Slot::Phase::Settled;      // (before the redo: the flags are looked at once even when it fails)
    if (check) {
        const int rc = redo_overflowed(c, s);
        if (rc) return rc;
    }
    if (copy == Copy::Complete && s.copy_pending) {
        HIP_TRY(hipStreamSynchronize(s.copy_stream.get()));
        if (c->fallbacks_fe != redone) {
            const int rc = enqueue_copy(c, s);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(s.copy_stream.get()));
        }
        finish_readback(c, s, s.copy);
        s.copy_pending = false;
    }
    return DG_OK;
}

namespace {

// Taking the slot for a new submission: what is in flight is finished first, a pending asynchronous readback included (it reads the
// framebuffer the new submission overwrites).  After that the slot is the builder's.
int take_slot(dg_ctx *c, Slot &s) {
    return s.phase == Slot::Phase::Queued || s.copy_pending ? make_final(c, s, Copy::Complete) : DG_OK;
}

// What a submission built for the slot leaves for later: whether it came from views, and then a copy of what they brought (the
// caller's arrays need not outlive the call).  The one place that writes the slot's kept copy.
void built_from(Slot &s, const dg_view *views, const BatchInputs &in, int n) {
    s.from_views = views != nullptr;
    s.kept.keep(views ? in : BatchInputs{}, n);
}

// Slot `slot` for a new submission of n views (or of the caller's lists), and its kernels enqueued.
int submit(dg_ctx *c, int slot, const dg_view *views, const dg_frame_lists *given, int n, const BatchInputs &in) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    int rc = take_slot(c, s);
    if (rc) return rc;
    rc = build_batch(c, s, views, given, n, in);
    if (rc) return rc;
    built_from(s, views, in, n);
    return enqueue_kernels(c, s);
}

// The synchronous calls' tail, given what their submission returned: its results through `read` when an output was handed over, or
// just its end.
template <class Read>
int read_or_wait(dg_ctx *c, int slot, int rc, bool wanted, Read read) {
    if (rc) return rc;
    return wanted ? read() : dg_wait(c, slot);
}
int read_or_wait(dg_ctx *c, int slot, int rc, int n, uint8_t *out) {
    return read_or_wait(c, slot, rc, out != nullptr, [&] { return dg_readback(c, slot, 0, n, out); });
}

// What a submission with a label part needs of the slot: the owner tags' staging and HBM, and a box table for the scene's map objects.
int ensure_label_buffers(dg_ctx *c, Slot &s) {
    const size_t n_mobjs = c->scene->mobjs.size();
    if (!s.d_owners) {
        HIP_TRY(hip_alloc(s.h_owners, std::max<size_t>(c->wall_cap_per_batch, 4) * sizeof(uint32_t)));
        HIP_TRY(hip_alloc(s.d_owners, std::max<size_t>(c->wall_cap_per_batch, 4) * sizeof(uint32_t)));
    }
    if (!s.per_scene.d_boxes) {
        HIP_TRY(hip_alloc(s.per_scene.d_boxes, std::max<size_t>((size_t)c->cfg.max_batch * n_mobjs, 1) * sizeof(LabelRawBox)));
        s.per_scene.box_mobjs = n_mobjs;
    }
    return DG_OK;
}

// Where the plane kernels write the slot's submission: the parts it holds, at their places in the framebuffer slab.
BundlePlanes planes_of(const dg_ctx *c, Slot &s) {
    const BundleLayout L = s.layout((size_t)c->cfg.width, (size_t)c->cfg.height);
    uint8_t *const fb = s.d_fb.get();
    BundlePlanes out{};
    if (s.holds(BUNDLE_DEPTH)) { out.dist = reinterpret_cast<int16_t *>(fb + L.distance); out.kind = fb + L.kind; }
    if (s.holds(BUNDLE_LABELS)) {
        out.id = reinterpret_cast<uint16_t *>(fb + L.id); out.cls = fb + L.cls;
        out.boxes = s.per_scene.d_boxes.get(); out.n_mobjs = (uint32_t)s.per_scene.box_mobjs;
    }
    return out;
}

// A depth or label submission's launch on the slot's own stream has returned e.
int launched(Slot &s, hipError_t e, const char *what) {
    if (e == hipSuccess) return queued(s);
    s.reset();                                            // (as a failed enqueue_kernels: the slot is left empty)
    return set_err(DG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Slot `slot` for a depth submission of n views (or of the caller's lists): always the host list path, whatever front end the ctx has;
// dg_depth_tiles on the slot's own stream, behind the upload.
int submit_depth(dg_ctx *c, int slot, const dg_view *views, const dg_frame_lists *given, int n, const BatchInputs &in) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    int rc = take_slot(c, s);
    if (rc) return rc;
    rc = build_batch_host(c, s, views, given, n, in, DG_FE_DEPTH);
    if (rc) return rc;
    built_from(s, views, in, n);
    const BundlePlanes out = planes_of(c, s);
    return launched(s, launch_depth(s.P, out.dist, out.kind, s.stream.get(), s.ev_rstart.get(), s.ev_raster.get()), "launch_depth");
}

// Slot `slot` for a label submission of n views (or of the caller's lists with their owner tags): the host list path like depth;
// dg_label_tiles and dg_label_boxes on the slot's own stream, behind the uploads.  ev_setup, which a label submission has no front-end
// half to time with, marks the end of dg_label_tiles.
int submit_labels(dg_ctx *c, int slot, const dg_view *views, const dg_frame_lists *given, const uint32_t *const *owners, int n, const BatchInputs &in) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    int rc = take_slot(c, s);
    if (rc) return rc;
    if (const int bad = check_batch(c, n)) return bad;
    std::string err;
    if ((rc = check_label_scene(*c->scene, err))) return set_err(rc, err);
    if ((rc = ensure_label_buffers(c, s))) return rc;
    rc = build_batch_host(c, s, views, given, n, in, DG_FE_LABELS, owners);
    if (rc) return rc;
    built_from(s, views, in, n);
    const BundlePlanes out = planes_of(c, s);
    return launched(s, launch_labels(s.P, s.d_owners.get(), out.id, out.cls, out.boxes, out.n_mobjs, s.stream.get(), s.ev_rstart.get(), s.ev_setup.get(), s.ev_raster.get()), "launch_labels");
}

int check_bundle_what(uint32_t what) {
    if (what == 0 || (what & ~BUNDLE_ALL)) return set_err(DG_ERR_INVALID, "what must be a non-empty set of DG_BUNDLE_COLOUR, DG_BUNDLE_DEPTH, DG_BUNDLE_LABELS");
    return DG_OK;
}

int bundle_capacity_of(const dg_ctx *c, uint32_t what) {
    return (int)bundle_capacity((size_t)c->cfg.max_batch, (size_t)c->cfg.width, (size_t)c->cfg.height, what);
}

// The kernels of the bundle the slot describes (build_batch_host has queued its uploads on the slot's stream), on the ctx's kernel
// stream behind every earlier submission's, as enqueue_kernels does: the colour kernels of the host list route when colour is asked
// for — P.fb is the slab's base — then the clearing of the box rows and dg_bundle_tiles when a plane is.  ev_raster goes to whichever
// kernel is the last.  A HIP call that fails half way leaves the slot empty.
int enqueue_bundle(dg_ctx *c, Slot &s) {
    hipStream_t ks = c->kstream.get();
    Invalidate guard{s};
    const uint32_t what = s.bundle_what;
    const bool colour = (what & BUNDLE_COLOUR) != 0, tiles = (what & (BUNDLE_DEPTH | BUNDLE_LABELS)) != 0;
    if (const int rc = after_upload(s, ks)) return rc;
    if (colour) {
        HIP_TRY(launch_setup(s.P, s.max_spans, ks, s.ev_start.get(), s.ev_setup.get()));
        HIP_TRY(launch_raster(s.P, ks, s.ev_rstart.get(), tiles ? s.ev_cend.get() : s.ev_raster.get()));
    }
    if (tiles) HIP_TRY(launch_bundle(s.P, s.d_owners.get(), planes_of(c, s), what, ks, s.ev_tiles.get(), s.ev_raster.get()));
    guard.armed = false;
    return queued(s);                                     // (never DG_FE_AUTO's measurement)
}

// Slot `slot` for a bundle of n views (or of the caller's lists, with their owner tags when labels are asked for): the host list path
// whatever front end the ctx has, one list build and one upload for every part.
int submit_bundle(dg_ctx *c, int slot, const dg_view *views, const dg_frame_lists *given, const uint32_t *const *owners, int n, const BatchInputs &in,
                  uint32_t what) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    if (const int bad = check_batch(c, n)) return bad;
    if (n > bundle_capacity_of(c, what)) return set_err(DG_ERR_CAPACITY, "bundle: the parts of that many views do not fit the slot's framebuffer slab (dg_bundle_capacity)");
    const bool labels = (what & BUNDLE_LABELS) != 0;
    std::string err;
    int rc;
    if (labels && (rc = check_label_scene(*c->scene, err))) return set_err(rc, err);
    if ((rc = take_slot(c, s))) return rc;
    if (labels && (rc = ensure_label_buffers(c, s))) return rc;
    rc = build_batch_host(c, s, views, given, n, in, DG_FE_BUNDLE, owners, labels);
    if (rc) {
        if (s.phase == Slot::Phase::Prepared && s.front_end == DG_FE_BUNDLE) s.reset();   // (described, then an upload failed: nothing says yet which parts it has)
        return rc;
    }
    built_from(s, views, in, n);
    s.bundle_what = what;
    return enqueue_bundle(c, s);
}

// check_view_inputs for every view of a batch.  (Only the surfaces' message names the frame.)
int check_batch_inputs(const BatchInputs &in, int n) {
    std::string why;
    for (int i = 0; in.any() && i < n; i++)
        if (!check_view_inputs(in.at(i), why)) return set_err(DG_ERR_INVALID, (why == view_surfaces_error(32u) ? "frame " + std::to_string(i) + ": " : "") + why);
    return DG_OK;
}

// The slot's mask rows (max_batch x words), there from its first submission with a mask after dg_upload_scene on.
int ensure_slot_masks(dg_ctx *c, Slot &s, size_t words) {
    Slot::PerScene &b = s.per_scene;
    if (b.d_masks) return DG_OK;
    HIP_TRY(slot_sync(s));                                // (the slot is ours: whatever replayed the old rows has finished)
    HIP_TRY(hip_alloc(b.h_masks, (size_t)c->cfg.max_batch * words * sizeof(uint32_t)));
    HIP_TRY(hip_alloc(b.d_masks, (size_t)c->cfg.max_batch * words * sizeof(uint32_t)));
    b.mask_words = words;
    return DG_OK;
}

// The slot's floor cells and sector rows (max_batch x sectors), there from its first floor-textured submission after dg_upload_scene on.
int ensure_slot_floor(dg_ctx *c, Slot &s) {
    Slot::PerScene &b = s.per_scene;
    if (b.d_floor_cells) return DG_OK;
    HIP_TRY(slot_sync(s));
    const size_t cells = (size_t)c->cfg.max_batch * c->scene->sectors.size();
    HIP_TRY(hip_alloc(b.h_floor_cells, cells * sizeof(FloorCell)));
    HIP_TRY(hip_alloc(b.d_floor_seen, (size_t)c->cfg.max_batch * floor_seen_words(*c->scene) * sizeof(uint32_t)));
    HIP_TRY(hip_alloc(b.d_floor_cells, cells * sizeof(FloorCell)));
    return DG_OK;
}

// The slot's things block (staging + HBM) holds at least `bytes`: there from its first *_things submission after dg_upload_scene on, and
// grown (never shrunk) when a submission brings more pose entries than any before it.
int ensure_slot_things(dg_ctx *c, Slot &s, size_t bytes) {
    Slot::PerScene &b = s.per_scene;
    if (b.d_things && b.things_cap >= bytes) return DG_OK;
    HIP_TRY(slot_sync(s));
    const size_t cap = std::max<size_t>(bytes + bytes / 2, 256);
    b.things_cap = 0;
    HIP_TRY(hip_alloc(b.h_things, cap));
    HIP_TRY(hip_alloc(b.d_things, cap));
    b.things_cap = cap;
    return DG_OK;
}

// What a *_things submission ships: n rows of shown bits, the entry index first[n + 1] and the frames' sorted pose entries, in one block.
struct ThingBatch {
    std::vector<uint8_t> block;
    size_t first_at = 0, entries_at = 0;
};

// Every view's rows and entries of a *_things submission (thing_view_rows), with every check of its states and poses: the block as the
// kernels read it.  The ctx's marker table does not fit the scene, or there is none: rows of no words and no entries.
int build_thing_batch(dg_ctx *c, const dg_view *views, int n, const dg_view_state *states, const dg_view_poses *poses, ThingBatch &out) {
    const Scene &sc = *c->scene;
    std::string err;
    int rc = thing_check_call(sc, err);
    if (rc) return set_err(rc, err);
    const std::vector<dg_map_marker> *markers = thing_markers(sc, c->markers);
    const size_t words = markers ? thing_shown_words((uint32_t)sc.mobjs.size()) : 0;
    static thread_local std::vector<uint32_t> rows, first;
    static thread_local std::vector<ThingEntry> entries;
    static thread_local ThingViewScratch scratch;
    rows.assign((size_t)n * words, 0u);
    first.assign((size_t)n + 1, 0u);
    entries.clear();
    for (int i = 0; i < n; i++) {
        first[(size_t)i] = (uint32_t)entries.size();
        const ViewInputs in{states ? states + i : nullptr, poses ? poses + i : nullptr};
        if (!markers) rc = check_view_inputs(in, err) ? DG_OK : DG_ERR_INVALID;
        else {
            dg_view v = views[i];
            fill_view_trig(v);
            rc = thing_view_rows(sc, *markers, &c->fx.mobj, v, in.state, in.poses, scratch, rows.data() + (size_t)i * words, entries, err);
        }
        if (rc) return set_err(rc, "frame " + std::to_string(i) + ": " + err);
        if (entries.size() > 0x7fffffffu) return set_err(DG_ERR_CAPACITY, "map markers: too many pose entries in one submission");
    }
    first[(size_t)n] = (uint32_t)entries.size();
    out.first_at = rows.size() * sizeof(uint32_t);
    out.entries_at = out.first_at + first.size() * sizeof(uint32_t);
    out.block.resize(out.entries_at + std::max<size_t>(entries.size(), 1) * sizeof(ThingEntry));
    if (!rows.empty()) std::memcpy(out.block.data(), rows.data(), out.first_at);
    std::memcpy(out.block.data() + out.first_at, first.data(), first.size() * sizeof(uint32_t));
    if (!entries.empty()) std::memcpy(out.block.data() + out.entries_at, entries.data(), entries.size() * sizeof(ThingEntry));
    return DG_OK;
}

// What the map submissions do alike once each has checked its own arguments: slot `slot` for n map frames of kind fe, and their
// kernels enqueued.  arrow_lines(v, l, err): the kind's per-view checks and the arrow's three lines of view v (trig filled; the host owns
// the libm trig: dg_view has no field for the head angles) into l, which starts as three empty lines.  ego: a player-centred submission's
// parameters (else null): its views follow the arrow lines.  mask: n rows of the scene's row length, or null.  cells: a floor-textured
// submission's n rows of floor cells (else null).  things: a *_things submission's block (else null).
template <class ArrowLines>
int submit_map_frames(dg_ctx *c, int slot, int32_t fe, const dg_view *views, int n, const dg_ego_map *ego, const uint32_t *mask, ArrowLines arrow_lines,
                      const FloorCell *cells = nullptr, const ThingBatch *things = nullptr) {
    const int W = c->cfg.width, H = c->cfg.height;
    const size_t words = seen_words((uint32_t)c->scene->linedefs.size());
    const size_t bytes = ego_views_at(n) + (ego ? (size_t)n * sizeof(EgoView) : 0), mask_bytes = mask ? (size_t)n * words * sizeof(uint32_t) : 0;
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    int rc = take_slot(c, s);
    if (rc) return rc;
    if (bytes > s.lists_cap) return set_err(DG_ERR_CAPACITY, "list slab too small");
    if (mask && (rc = ensure_slot_masks(c, s, words))) return rc;
    if (cells && (rc = ensure_slot_floor(c, s))) return rc;
    if (things && (rc = ensure_slot_things(c, s, things->block.size()))) return rc;
    const size_t thing_bytes = things ? things->block.size() : 0;
    const size_t cell_bytes = cells ? (size_t)n * c->scene->sectors.size() * sizeof(FloorCell) : 0;
    const auto t0 = std::chrono::steady_clock::now();
    MapSeg *h = reinterpret_cast<MapSeg *>(s.h_lists.get());
    EgoView *hv = reinterpret_cast<EgoView *>(s.h_lists.get() + ego_views_at(n));
    std::string err;
    for (int i = 0; i < n; i++) {
        dg_view v = views[i];
        fill_view_trig(v);
        dg_map_line l[3] = {};
        rc = arrow_lines(v, l, err);
        if (rc) return set_err(rc, "frame " + std::to_string(i) + ": " + err);
        for (int k = 0; k < 3; k++) h[3 * i + k] = map_seg_make(l[k].x0, l[k].y0, l[k].x1, l[k].y1, l[k].rgb, W, H);   // clipped to the frame
        if (ego) hv[i] = ego_view(v);
    }
    if (mask) std::memcpy(s.per_scene.h_masks.get(), mask, mask_bytes);
    if (cells) std::memcpy(s.per_scene.h_floor_cells.get(), cells, cell_bytes);
    if (things) std::memcpy(s.per_scene.h_things.get(), things->block.data(), thing_bytes);
    s.map = Slot::MapState{ego ? *ego : dg_ego_map{}, mask != nullptr, false, things != nullptr, things ? things->first_at : 0, things ? things->entries_at : 0};
    s.describe(fe, n, bytes + mask_bytes + cell_bytes + thing_bytes, 0, 0);
    built_from(s, nullptr, BatchInputs{}, n);
    s.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(hipMemcpyAsync(s.d_lists.get(), s.h_lists.get(), bytes, hipMemcpyHostToDevice, s.stream.get()));
    if (mask) HIP_TRY(hipMemcpyAsync(s.per_scene.d_masks.get(), s.per_scene.h_masks.get(), mask_bytes, hipMemcpyHostToDevice, s.stream.get()));
    if (cells) HIP_TRY(hipMemcpyAsync(s.per_scene.d_floor_cells.get(), s.per_scene.h_floor_cells.get(), cell_bytes, hipMemcpyHostToDevice, s.stream.get()));
    if (things) HIP_TRY(hipMemcpyAsync(s.per_scene.d_things.get(), s.per_scene.h_things.get(), thing_bytes, hipMemcpyHostToDevice, s.stream.get()));
    return enqueue_kernels(c, s);
}

}  // namespace

extern "C" {

int dg_create(const dg_config *cfg, dg_ctx **out) {
    if (!cfg || !out) return set_err(DG_ERR_INVALID, "null argument");
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 16384 || cfg->height > 16384)
        return set_err(DG_ERR_INVALID, "width/height must be positive, both <= 16384");
    if (cfg->max_batch <= 0 || cfg->max_batch > 65535 || cfg->slots <= 0 || cfg->slots > 16)
        return set_err(DG_ERR_INVALID, "max_batch must be in [1, 65535], slots in [1, 16]");
    if (cfg->front_end < DG_FE_AUTO || cfg->front_end > DG_FE_DEVICE_SEGS) return set_err(DG_ERR_INVALID, "front_end must be DG_FE_AUTO, DG_FE_HOST, DG_FE_DEVICE or DG_FE_DEVICE_SEGS");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_err(DG_ERR_NO_DEVICE, "no HIP device (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return set_err(DG_ERR_NO_DEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(DG_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    HIP_TRY(hipSetDevice(cfg->device));

    std::unique_ptr<dg_ctx> c(new dg_ctx());     // (an error below destroys it half built: ~dg_ctx)
    c->cfg = *cfg;
    c->fk = make_consts(cfg->width, cfg->height);
    c->dk = DevConsts{c->fk.ARC, c->fk.GCFX, c->fk.CFX, c->fk.CFY, cfg->width, cfg->height};
    // Default: the process's CPU share — its affinity mask and, in a container, its cgroup CPU quota (threads beyond the quota only get
    // the process throttled) — capped at 16 per ctx: an 8-GPU node gives each rank ~1/8 of the cores.
    int nthreads = cfg->host_threads;
    if (nthreads <= 0) {
        cpu_set_t set;
        CPU_ZERO(&set);
        int avail = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        const int quota = cgroup_cpu_quota();
        if (quota > 0) avail = std::min(avail, quota);
        nthreads = std::max(1, std::min(avail, 16));
    }
    nthreads = std::min(nthreads, 256);
    c->n_threads = nthreads;
    c->pool.reset(new Pool(nthreads - 1));
    for (int i = 0; i < nthreads; i++) c->arenas.emplace_back(new FrameArena());
    c->binned.resize((size_t)cfg->max_batch);

    const size_t W = (size_t)cfg->width, H = (size_t)cfg->height, F = (size_t)cfg->max_batch;
    c->span_cap_per_batch = F * W * 24;       // 24 spans per column on average; real scenes use 2-8
    c->wall_cap_per_batch = F * 4096;
    c->plane_cap_per_batch = F * 4096;
    // (the slabs' capacities: the layouts at the caps, plus slack)
    const size_t lists_cap = list_layout(F, W, c->wall_cap_per_batch, c->plane_cap_per_batch, c->span_cap_per_batch).total + 1024;
    c->fe_enabled = cfg->front_end != DG_FE_HOST;
    c->fs_enabled = cfg->front_end == DG_FE_DEVICE_SEGS || cfg->front_end == DG_FE_AUTO;
    c->fs_forced = cfg->front_end == DG_FE_DEVICE_SEGS;
    if (c->fe_enabled) {
        // Scratch slots per screen column (spans and wall-record columns).  A column that needs more sends its batch through
        // the host list path; DOOMGPU_FE_COLUMN_SLOTS trades scratch HBM (24 B x slots x width x max_batch) against that.
        if (const char *e = std::getenv("DOOMGPU_FE_COLUMN_SLOTS")) {
            const long v = std::strtol(e, nullptr, 10);
            if (v >= 1 && v <= (long)FE_MAX_COL_SLOTS) c->fe_col_slots = (uint32_t)v;
        }
        c->fe_out.resize(F);
        size_t parts_per_frame = 2048;     // wall records per frame on average (e1m1-like maps ship 20-200 after culling)
        if (const char *e = std::getenv("DOOMGPU_FE_RECORDS_PER_FRAME")) {   // sizes the record slab; a batch that needs more goes through the host list path
            const long v = std::strtol(e, nullptr, 10);
            if (v >= 1 && v <= 65535) parts_per_frame = (size_t)v;
        }
        c->fe_part_cap = F * parts_per_frame;
        c->fe_sprite_cap = F * 256;
        c->fe_behind_cap = F * 256 * 32;   // one bit per (sprite, wall record)
        c->fe_bin_cap = F * 16384;         // column-bin entries (a record is listed in every 64-column strip it touches)
        c->fe_sbin_cap = F * 2048;
        c->fe_slab_cap = fe_layout(F, W, c->fe_part_cap, c->fe_sprite_cap, c->fe_behind_cap, F * FE_MAX_SKY_SLOTS, c->fe_bin_cap, c->fe_sbin_cap).total + 1024;
    }
    c->slots.resize((size_t)cfg->slots);
    HIP_TRY(hip_alloc(c->d_checksums, F * 8));
    if (c->fe_enabled) {
        HIP_TRY(hip_alloc(c->d_fe_cspans, F * c->fe_col_slots * W * sizeof(FeU4)));
        HIP_TRY(hip_alloc(c->d_fe_recs, F * c->fe_col_slots * W * sizeof(FeColRec)));
        HIP_TRY(hip_alloc(c->d_fe_cnt, F * W * 4));
    }
    {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(stream_create(c->kstream, &hi));
        // Small frames: the front-end kernels of a batch are chains of dependent steps that leave most of the chip idle, and at 320x200 they
        // last as long as the raster launch itself — letting the next batch's front end run next to this batch's raster launch (two streams,
        // tied by the front end's last dispatch event) is worth 17 % there (2.57 -> 3.02 M frames/s), 7 % at 640x400, 2 % at 800x600.  From 1024x768 up the raster launch
        // fills the chip and the overlap costs 1-2 % (profiles/r03_column_walk.md, r05_seg_walk.md).  DOOMGPU_RASTER_OVERLAP=0 / 1 overrides.
        c->raster_overlap = (size_t)cfg->width * (size_t)cfg->height <= kOverlapMaxPixels;
        if (const char *e = std::getenv("DOOMGPU_RASTER_OVERLAP")) c->raster_overlap = std::atoi(e) != 0;
        if (c->raster_overlap) HIP_TRY(stream_create(c->rstream, &hi));
    }
    for (Slot &s : c->slots) {
        HIP_TRY(stream_create(s.stream));
        for (Event *ev : {&s.ev_start, &s.ev_setup, &s.ev_raster, &s.ev_rstart, &s.ev_cend, &s.ev_tiles, &s.pose_run.t0, &s.pose_run.t1, &s.height_run.t0, &s.height_run.t1, &s.flat_run.t0, &s.flat_run.t1}) HIP_TRY(event_create(*ev));
        HIP_TRY(event_create(s.ev_h2d, false));            // (it only orders streams)
        HIP_TRY(stream_create(s.copy_stream));
        HIP_TRY(hip_alloc(s.h_lists, lists_cap));
        HIP_TRY(hip_alloc(s.d_lists, lists_cap));
        HIP_TRY(hip_alloc(s.d_rspans, c->span_cap_per_batch * sizeof(DevRSpan)));
        HIP_TRY(hip_alloc(s.d_fb, F * 3 * W * H));
        if (c->fe_enabled) {
            HIP_TRY(hip_alloc(s.h_fe, c->fe_slab_cap));
            HIP_TRY(hip_alloc(s.d_fe, c->fe_slab_cap));
            HIP_TRY(hip_alloc(s.d_fe_coloff, F * (W + 1) * 4));
            HIP_TRY(hip_alloc(s.d_order, FS_ORDER_CLASSES * F * fe_col_groups(W) * 4));
            SlabCursor ws;
            ws.take(F * 4 + FS_ORDER_CLASSES * 4);                              // the flag words, then the seg walk's launch-order counters
            const size_t off_events = ws.take(F * FE_MAX_SKY_SLOTS * 3 * ((W + 63) / 64) * 8);
            s.walk_state_bytes = ws.end();
            HIP_TRY(hip_alloc(s.d_flags, s.walk_state_bytes));
            s.d_events = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(s.d_flags.get()) + off_events);
            HIP_TRY(hip_alloc(s.h_status, 2 * F * 4));
        }
        s.lists_cap = lists_cap;
    }
    *out = c.release();
    return DG_OK;
}

void dg_destroy(dg_ctx *ctx) { delete ctx; }
int dg_ctx_host_threads(const dg_ctx *ctx) { return ctx ? ctx->n_threads : DG_ERR_INVALID; }

int dg_upload_scene(dg_ctx *c, const dg_scene *scene) {
    if (!c || !scene) return set_err(DG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    for (Slot &s : c->slots) {             // nothing may still read the old scene or write into a buffer a pending readback is copying from
        // A slot with work in flight is FINISHED against the scene it was rendered from (still resident): a device-walk batch that
        // overflowed a capacity is redone and its pending readback re-issued, exactly as dg_wait would have done.  (If that redo is
        // impossible — the old scene object itself was changed since its upload — the slot is just drained.)
        if (c->scene) (void)take_slot(c, s);
        HIP_TRY(slot_sync(s));
        HIP_TRY(hipStreamSynchronize(s.copy_stream.get()));
        if (s.copy_pending) finish_readback(c, s, s.copy);     // (a slot that was only drained: its copies have run all the same)
        s.copy_pending = false;
    }
    const Scene &sc = *scene->sc;
    c->d_palette.reset(); c->d_texel_idx.reset(); c->d_texel_opq.reset();
    c->d_flats = nullptr;               // inside d_texel_idx's allocation
    c->pictures.clear();                // (their texels went with the planes)
    // the slots' prepared records point into the device scene that was just freed: nothing may be replayed from them
    for (Slot &s : c->slots) { s.reset(); s.per_scene.drop(); }                   // (the box table is sized by the scene's map objects, a mask row by its linedefs)
    // ... and what was derived from the old scene goes (a new scene may reuse the old one's address and revision).  The slots are drained;
    // dg_seen_lines_device, dg_slot_seen_lines and dg_ctx_locate_walks are synchronous: nothing of them is in flight.
    c->per_scene.drop();
    uint32_t pal[256];
    for (int i = 0; i < 256; i++) pal[i] = (uint32_t)sc.palette[3 * i] | ((uint32_t)sc.palette[3 * i + 1] << 8) | ((uint32_t)sc.palette[3 * i + 2] << 16);
    const size_t nt = std::max<size_t>(sc.texel_idx.size(), 16), nf = std::max<size_t>(sc.flat_pool.size(), 16);
    float palf[256 * 4];
    for (int i = 0; i < 256; i++) { palf[4 * i] = (float)sc.palette[3 * i]; palf[4 * i + 1] = (float)sc.palette[3 * i + 1]; palf[4 * i + 2] = (float)sc.palette[3 * i + 2]; palf[4 * i + 3] = 0.0f; }
    HIP_TRY(hip_alloc(c->d_palette, sizeof pal + sizeof palf));
    // [column-major texel index plane | flats] share one allocation: the tile rasteriser gathers every kind's texel with one
    // 32-bit offset from texel_idx (flats at flats - texel_idx)
    const size_t flats_at = (nt + 255) & ~(size_t)255;
    HIP_TRY(hip_alloc(c->d_texel_idx, flats_at + nf));
    HIP_TRY(hip_alloc(c->d_texel_opq, nt));
    c->d_flats = c->d_texel_idx.get() + flats_at;
    HIP_TRY(hipMemcpy(c->d_palette.get(), pal, sizeof pal, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_palette.get() + 256, palf, sizeof palf, hipMemcpyHostToDevice));
    if (!sc.texel_idx.empty()) {
        HIP_TRY(hipMemcpy(c->d_texel_idx.get(), sc.texel_idx.data(), sc.texel_idx.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_texel_opq.get(), sc.texel_opq.data(), sc.texel_opq.size(), hipMemcpyHostToDevice));
    }
    if (!sc.flat_pool.empty()) HIP_TRY(hipMemcpy(c->d_flats, sc.flat_pool.data(), sc.flat_pool.size(), hipMemcpyHostToDevice));
    const BitmapInfo &sky = sc.bitmaps[(size_t)sc.sky_bitmap];
    c->dscene = DevScene{c->d_palette.get(), reinterpret_cast<const float *>(c->d_palette.get() + 256), c->d_texel_idx.get(), c->d_texel_opq.get(), c->d_flats, sky.texel_off, sky.w, sky.h, sky.has_holes};
    if (!c->d_row_tab) HIP_TRY(hip_alloc(c->d_row_tab, (size_t)c->cfg.height * sizeof(uint4)));
    HIP_TRY(launch_row_table(c->dscene, c->dk, c->d_row_tab.get(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    c->scene = &sc;
    c->fx = sc.fx;                                      // the effects' setters (and dg_scene_mobj_event) take effect here
    c->markers = sc.markers;
    c->fe_scene_ok = sky.w >= 256 && sky.h >= 128;    // a smaller sky bitmap is an index panic only when a sky visplane is drawn: host path
    c->uploaded_texels = sc.texel_idx.size();
    c->pictures = overlay_pictures(sc);
    c->uploaded_flats = sc.flat_pool.size(); c->uploaded_anims = sc.anim.size();
    c->fs_scene_ok = false;
    if (c->fs_enabled && c->fe_scene_ok && sc.fs_ok && c->cfg.width <= FS_MAX_W) {
        const int rc = upload_fs_scene(c, sc);
        if (rc && c->fs_forced) return rc;                 // (DG_FE_AUTO simply keeps the host walker when the seg walk's memory cannot be had)
        if (rc) {
            static bool said = false;                      // once per process: the ctx works, but not the way it was asked to
            if (!said) { said = true; std::fprintf(stderr, "doomgpu: DG_FE_AUTO keeps the per-seg half on the host: no device memory for the seg walk's per-batch rows (%d views x %zu segs)\n", c->cfg.max_batch, sc.segs.size()); }
            drop_fs_scene(c);
            c->fs_scene_ok = false;
            (void)hipGetLastError();
        }
    }
    return DG_OK;
}

int dg_submit_views(dg_ctx *c, int slot, const dg_view *views, int n) { return dg_submit_views_state(c, slot, views, nullptr, n); }

int dg_render_views_state(dg_ctx *c, const dg_view *views, const dg_view_state *states, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_views_state(c, 0, views, states, n), n, out);
}

int dg_submit_views_state(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, int n) {
    return dg_submit_views_poses(c, slot, views, states, nullptr, n);
}

int dg_submit_views_poses(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n) {
    return dg_submit_views_sectors(c, slot, views, states, poses, nullptr, n);
}

int dg_submit_views_sectors(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n) {
    return dg_submit_views_surfaces(c, slot, views, states, poses, sectors, nullptr, n);
}

int dg_submit_views_surfaces(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors,
                             const dg_view_surfaces *surfaces, int n) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    const BatchInputs in{states, poses, sectors, surfaces};
    if ((rc = check_batch_inputs(in, n))) return rc;
    return submit(c, slot, views, nullptr, n, in);
}

int dg_render_views_surfaces(dg_ctx *c, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors,
                             const dg_view_surfaces *surfaces, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_views_surfaces(c, 0, views, states, poses, sectors, surfaces, n), n, out);
}

int dg_render_views_sectors(dg_ctx *c, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_views_sectors(c, 0, views, states, poses, sectors, n), n, out);
}

int dg_render_views_poses(dg_ctx *c, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_views_poses(c, 0, views, states, poses, n), n, out);
}

int dg_wait(dg_ctx *c, int slot) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    return make_final(c, c->slots[(size_t)slot], Copy::Complete);
}

int dg_ctx_redone_frames(const dg_ctx *c, uint64_t *frames) {
    if (!c || !frames) return set_err(DG_ERR_INVALID, "null argument");
    *frames = c->redone_frames;
    return DG_OK;
}

int dg_ctx_fallbacks(const dg_ctx *c, uint64_t *front_end) {
    if (!c || !front_end) return set_err(DG_ERR_INVALID, "null argument");
    *front_end = c->fallbacks_fe;
    return DG_OK;
}

void *dg_alloc_host(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void dg_free_host(void *p) { if (p) (void)hipHostFree(p); }

int dg_render_views(dg_ctx *c, const dg_view *views, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_views(c, 0, views, n), n, out);
}

int dg_prepare_views(dg_ctx *c, int slot, const dg_view *views, int n) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    HIP_TRY(hipSetDevice(c->cfg.device));
    Slot &s = c->slots[(size_t)slot];
    rc = take_slot(c, s);
    if (rc) return rc;
    c->preparing = true;
    rc = build_batch(c, s, views, nullptr, n, BatchInputs{});
    c->preparing = false;
    if (rc) return rc;
    built_from(s, views, BatchInputs{}, n);
    if (s.column_walk()) {        // run the column walk once so that a batch that has to go through the host list path as a whole
        rc = enqueue_kernels(c, s);   // is re-prepared that way now, not on a replay
        if (rc) return rc;
    }
    return make_final(c, s, Copy::Leave);         // host lists: uploaded, and the slot stays prepared
}

int dg_replay_slot(dg_ctx *c, int slot) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    Slot &s = c->slots[(size_t)slot];
    if (s.phase == Slot::Phase::Empty) return set_err(DG_ERR_INVALID, "slot has no prepared lists");
    if (s.holds_bundle()) return set_err(DG_ERR_INVALID, "dg_replay_slot: the slot holds a bundle (submit it again)");
    if ((rc = refuse_no_colour(s, "dg_replay_slot"))) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    // A dg_readback_async may still be reading the framebuffer these kernels are about to overwrite, and a column-walk submission that
    // was never waited for has its overflow flags looked at before the walk clears them.  A host-list submission still in flight is not
    // waited for: its lists simply run again behind it.
    if (s.copy_pending) rc = make_final(c, s, Copy::Complete);
    else if (s.unchecked()) rc = make_final(c, s, Copy::Leave);
    if (rc) return rc;
    return enqueue_kernels(c, s);  // (the overflow flags are looked at again: frames that overflowed are redone on every replay)
}

int dg_draw_lists(dg_ctx *c, int slot, const dg_frame_lists *frames, int n, uint8_t *out) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!frames) return set_err(DG_ERR_INVALID, "null frames");
    return read_or_wait(c, slot, submit(c, slot, nullptr, frames, n, BatchInputs{}), n, out);
}

int dg_submit_depth_views(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, int n) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    const BatchInputs in{states};
    if ((rc = check_batch_inputs(in, n))) return rc;
    return submit_depth(c, slot, views, nullptr, n, in);
}

int dg_render_depth_views(dg_ctx *c, const dg_view *views, const dg_view_state *states, int n, int16_t *distance, uint8_t *kind) {
    return read_or_wait(c, 0, dg_submit_depth_views(c, 0, views, states, n), distance || kind, [&] { return dg_readback_depth(c, 0, 0, n, distance, kind); });
}

int dg_depth_lists(dg_ctx *c, int slot, const dg_frame_lists *frames, int n, int16_t *distance, uint8_t *kind) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!frames) return set_err(DG_ERR_INVALID, "null frames");
    return read_or_wait(c, slot, submit_depth(c, slot, nullptr, frames, n, BatchInputs{}), distance || kind, [&] { return dg_readback_depth(c, slot, 0, n, distance, kind); });
}

int dg_submit_label_views(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, int n) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    const BatchInputs in{states};
    if ((rc = check_batch_inputs(in, n))) return rc;
    return submit_labels(c, slot, views, nullptr, nullptr, n, in);
}

int dg_render_label_views(dg_ctx *c, const dg_view *views, const dg_view_state *states, int n, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    return read_or_wait(c, 0, dg_submit_label_views(c, 0, views, states, n), id || cls || boxes, [&] { return dg_readback_labels(c, 0, 0, n, id, cls, boxes); });
}

int dg_label_lists(dg_ctx *c, int slot, const dg_frame_lists *frames, const uint32_t *const *owners, int n, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!frames || !owners) return set_err(DG_ERR_INVALID, "null frames or owners");
    return read_or_wait(c, slot, submit_labels(c, slot, nullptr, frames, owners, n, BatchInputs{}), id || cls || boxes, [&] { return dg_readback_labels(c, slot, 0, n, id, cls, boxes); });
}

int dg_bundle_capacity(const dg_ctx *c, uint32_t what) {
    if (!c) return set_err(DG_ERR_INVALID, "null ctx");
    const int rc = check_bundle_what(what);
    return rc ? rc : bundle_capacity_of(c, what);
}

int dg_submit_bundle_views(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, int n, uint32_t what) {
    return dg_submit_bundle_views_poses(c, slot, views, states, nullptr, n, what);
}

int dg_submit_bundle_views_poses(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n, uint32_t what) {
    return dg_submit_bundle_views_sectors(c, slot, views, states, poses, nullptr, n, what);
}

int dg_submit_bundle_views_sectors(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n,
                                   uint32_t what) {
    return dg_submit_bundle_views_surfaces(c, slot, views, states, poses, sectors, nullptr, n, what);
}

int dg_submit_bundle_views_surfaces(dg_ctx *c, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors,
                                    const dg_view_surfaces *surfaces, int n, uint32_t what) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    if ((rc = check_bundle_what(what))) return rc;
    const BatchInputs in{states, poses, sectors, surfaces};
    if ((rc = check_batch_inputs(in, n))) return rc;
    return submit_bundle(c, slot, views, nullptr, nullptr, n, in, what);
}

int dg_bundle_lists(dg_ctx *c, int slot, const dg_frame_lists *frames, const uint32_t *const *owners, int n, uint32_t what) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!frames) return set_err(DG_ERR_INVALID, "null frames");
    if ((rc = check_bundle_what(what))) return rc;
    if ((what & BUNDLE_LABELS) && !owners) return set_err(DG_ERR_INVALID, "null owners: DG_BUNDLE_LABELS needs the owner tags");
    rc = submit_bundle(c, slot, nullptr, frames, owners, n, BatchInputs{}, what);
    return rc ? rc : dg_wait(c, slot);                    // (no output of its own: the parts are the readbacks' to fetch)
}

int dg_submit_map_views(dg_ctx *c, int slot, const dg_view *views, int n) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views) return set_err(DG_ERR_INVALID, "null views");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const int W = c->cfg.width, H = c->cfg.height;
    if (W < 40 || H < 40) return set_err(DG_ERR_INVALID, "map frames need width and height >= 40");
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    return submit_map_frames(c, slot, DG_FE_MAP, views, n, nullptr, nullptr,
                             [&](const dg_view &v, dg_map_line *l, std::string &err) { return map_arrow_lines(*c->scene, W, H, v, l, err); });
}

int dg_render_map_views(dg_ctx *c, const dg_view *views, int n, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_map_views(c, 0, views, n), n, out);
}

int dg_submit_explored_map_views(dg_ctx *c, int slot, const dg_view *views, int n, const uint32_t *mask) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views || !mask) return set_err(DG_ERR_INVALID, "null views or mask");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const int W = c->cfg.width, H = c->cfg.height;
    if (W < 40 || H < 40) return set_err(DG_ERR_INVALID, "map frames need width and height >= 40");
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    const size_t words = seen_words((uint32_t)c->scene->linedefs.size());
    if (words > EXPLORED_MAX_WORDS) return set_err(DG_ERR_CAPACITY, "explored map frames: more than 65536 linedefs");
    if (words == 0) return set_err(DG_ERR_INVALID, "explored map frames: the scene has no linedefs");
    return submit_map_frames(c, slot, DG_FE_MAP_EXPLORED, views, n, nullptr, mask,
                             [&](const dg_view &v, dg_map_line *l, std::string &err) { return map_arrow_lines(*c->scene, W, H, v, l, err); });
}

int dg_render_explored_map_views(dg_ctx *c, const dg_view *views, int n, const uint32_t *mask, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_explored_map_views(c, 0, views, n, mask), n, out);
}

int dg_submit_ego_map_views(dg_ctx *c, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views || !params) return set_err(DG_ERR_INVALID, "null views or params");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const int W = c->cfg.width, H = c->cfg.height;
    std::string err;
    rc = ego_check_call(*c->scene, W, H, params, err);
    if (rc) return set_err(rc, err);
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    const bool arrow = (params->flags & EGO_ARROW) != 0;
    return submit_map_frames(c, slot, DG_FE_MAP_EGO, views, n, params, mask, [&](const dg_view &v, dg_map_line *l, std::string &why) {
        const int bad = ego_check_view(v, why);               // (the contract's checks, whether or not an arrow is drawn)
        return bad || !arrow ? bad : ego_arrow_lines(W, H, v, *params, l, why);
    });
}

int dg_render_ego_map_views(dg_ctx *c, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_ego_map_views(c, 0, views, n, params, mask), n, out);
}

// dg_submit_ego_map_views with the things block; every check of every view, its state and its poses comes before the slot is touched.
int dg_submit_ego_map_views_things(dg_ctx *c, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                                   const dg_view_poses *poses) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views || !params) return set_err(DG_ERR_INVALID, "null views or params");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const int W = c->cfg.width, H = c->cfg.height;
    std::string err;
    rc = ego_check_call(*c->scene, W, H, params, err);
    if (rc) return set_err(rc, err);
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    const bool arrow = (params->flags & EGO_ARROW) != 0;
    for (int i = 0; i < n; i++) {
        dg_view v = views[i];
        fill_view_trig(v);
        dg_map_line l[3] = {};
        rc = ego_check_view(v, err);
        if (!rc && arrow) rc = ego_arrow_lines(W, H, v, *params, l, err);
        if (rc) return set_err(rc, "frame " + std::to_string(i) + ": " + err);
    }
    static thread_local ThingBatch batch;
    rc = build_thing_batch(c, views, n, states, poses, batch);
    if (rc) return rc;
    return submit_map_frames(c, slot, DG_FE_MAP_EGO, views, n, params, mask, [&](const dg_view &v, dg_map_line *l, std::string &why) {
        return arrow ? ego_arrow_lines(W, H, v, *params, l, why) : DG_OK;
    }, nullptr, &batch);
}

int dg_render_ego_map_views_things(dg_ctx *c, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                                   const dg_view_poses *poses, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_ego_map_views_things(c, 0, views, n, params, mask, states, poses), n, out);
}

// dg_submit_floor_map_views and its *_things form.  Every check of the call and of every view comes before the slot is touched: the
// cells of all n views (and, with things, their rows and entries) are built first.
static int submit_floor_frames(dg_ctx *c, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                               const dg_view_surfaces *surfaces, bool things, const dg_view_poses *poses) {
    int rc = check_slot(c, slot);
    if (rc) return rc;
    if (!views || !params) return set_err(DG_ERR_INVALID, "null views or params");
    if (!c->scene) return set_err(DG_ERR_INVALID, "no scene uploaded (dg_upload_scene)");
    const Scene &sc = *c->scene;
    const int W = c->cfg.width, H = c->cfg.height;
    std::string err;
    rc = floor_check_call(sc, W, H, params, err);
    if (rc) return set_err(rc, err);
    if (n <= 0 || n > c->cfg.max_batch) return set_err(DG_ERR_CAPACITY, "batch size outside [1, max_batch]");
    if (sc.flat_pool.size() != c->uploaded_flats || sc.anim.size() != c->uploaded_anims) return set_err(DG_ERR_INVALID, "the scene loaded new flats since dg_upload_scene: upload it again");
    const bool arrow = (params->flags & EGO_ARROW) != 0;
    const size_t S = sc.sectors.size();
    static thread_local std::vector<FloorCell> cells;
    static thread_local FloorRowScratch scratch;
    static thread_local ThingBatch batch;
    cells.resize((size_t)n * S);
    for (int i = 0; i < n; i++) {
        dg_view v = views[i];
        fill_view_trig(v);
        dg_map_line l[3] = {};
        rc = ego_check_view(v, err);
        if (!rc && arrow) rc = ego_arrow_lines(W, H, v, *params, l, err);
        if (!rc) rc = floor_view_cells(sc, &c->fx.light, v, states ? states + i : nullptr, surfaces ? surfaces + i : nullptr, scratch, cells.data() + (size_t)i * S, err);
        if (rc) return set_err(rc, "frame " + std::to_string(i) + ": " + err);
    }
    if (things && (rc = build_thing_batch(c, views, n, states, poses, batch))) return rc;
    return submit_map_frames(c, slot, DG_FE_MAP_FLOOR, views, n, params, mask, [&](const dg_view &v, dg_map_line *l, std::string &why) {
        return arrow ? ego_arrow_lines(W, H, v, *params, l, why) : DG_OK;
    }, cells.data(), things ? &batch : nullptr);
}

int dg_submit_floor_map_views(dg_ctx *c, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                              const dg_view_surfaces *surfaces) {
    return submit_floor_frames(c, slot, views, n, params, mask, states, surfaces, false, nullptr);
}

int dg_submit_floor_map_views_things(dg_ctx *c, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                                     const dg_view_surfaces *surfaces, const dg_view_poses *poses) {
    return submit_floor_frames(c, slot, views, n, params, mask, states, surfaces, true, poses);
}

int dg_render_floor_map_views_things(dg_ctx *c, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                                     const dg_view_surfaces *surfaces, const dg_view_poses *poses, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_floor_map_views_things(c, 0, views, n, params, mask, states, surfaces, poses), n, out);
}

int dg_render_floor_map_views(dg_ctx *c, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, const dg_view_state *states,
                              const dg_view_surfaces *surfaces, uint8_t *out) {
    return read_or_wait(c, 0, dg_submit_floor_map_views(c, 0, views, n, params, mask, states, surfaces), n, out);
}

}  // extern "C"
