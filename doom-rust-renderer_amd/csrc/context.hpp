// context.hpp — what the files that implement the C-ABI's dg_ctx entry points share (context.cpp: a slot's way from one submission
// to the next; api_readback.cpp: what reads a slot; api_device.cpp: the calls that run on a stream of the ctx's own and return when
// done): Slot, dg_ctx, HIP_TRY, and the few slot helpers one of them needs of another, with the headers all need.  Private to csrc/.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/doomgpu.h"
#include "api_common.hpp"
#include "binner.hpp"
#include "fe_auto.hpp"
#include "fe_kernels.hpp"
#include "floor_map_core.h"
#include "frontend.hpp"
#include "fs_kernels.hpp"
#include "hip_mem.hpp"
#include "kernels.hpp"
#include "light_fx_kernels.hpp"
#include "mobj_fx_kernels.hpp"
#include "plane_kernels.hpp"
#include "pool.hpp"
#include "reduce_core.h"
#include "scene.hpp"
#include "sight_core.h"
#include "slab_layout.h"
#include "view_rows_kernels.hpp"
#include "walk_core.h"

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return set_err(DG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace dg {

// One kind of per-view rows through the seg walk (view_rows_core.h).  A slot's buffers of it, as view_row_layout<K>
// sizes them: the rows the kind's kernels write, and the de-duplicated entries' staging + HBM.  All three or none: a slot without
// them sends its batches that carry the kind through the host walker (build_batch_fs).
template <class K> struct RowBuffers {
    DevPtr<typename K::Elem> rows;
    PinnedPtr<typename K::Entry> h_entries;
    DevPtr<typename K::Entry> d_entries;
    explicit operator bool() const { return rows != nullptr; }
    void alloc(const ViewRowLayout &L) {
        if (hip_alloc(rows, L.rows) == hipSuccess && hip_alloc(h_entries, L.entries) == hipSuccess && hip_alloc(d_entries, L.entries) == hipSuccess) return;
        *this = RowBuffers{};
        (void)hipGetLastError();    // (not an error of the upload: the host walker stands in)
    }
};
// ... and what a slot's last submission has of the kind: the kernels' arguments (n_frames 0: not launched), and the events on their
// first and last dispatch — t0 only when the batch's start event did not go to them (enqueue_kernels).
template <class K> struct RowRun {
    ViewRowParams<K> P{};
    Event t0, t1;
    bool from_start = false;      // they were the batch's first kernels: their start is the slot's ev_start, not t0
    bool on() const { return P.n_frames > 0; }
};

struct Slot {
    Stream stream;
    // timing events, attached to the dispatches themselves (kernels.hpp): first / last front-end kernel, raster launch; ev_raster is also
    // what "the slot's kernels are done" is waited on
    Event ev_start, ev_setup, ev_rstart, ev_raster, ev_h2d;
    // bundles: the end of the colour raster launch when dg_bundle_tiles follows it (ev_raster is then that kernel's end: always the end of
    // the submission's LAST kernel), and dg_bundle_tiles' start
    Event ev_cend, ev_tiles;
    // ev_raster has been recorded at least once: slot_sync waits only on an event that has.  Not part of the phase below, because it is
    // a fact about the event, not about the submission: it stays true when the slot goes back to empty.
    bool raster_recorded = false;
    Stream copy_stream;   // dg_readback_async / dg_readback_reduced_async / dg_readback_planes_reduced_async: D2H of this slot's frames while another slot's kernels run
    // What a readback moves (api_readback.cpp): frames [first, first + count) to host memory `out`, as they are or reduced by `desc` on
    // the way; or (planes) the depth and label planes of those frames to the outputs that are there, as they are or reduced by `pdesc`
    // on the way, and their box rows
    struct Readback {
        uint8_t *out = nullptr;
        int first = 0, count = 0;
        bool reduced = false;            // goes through the slot's scratch (d_reduced)
        dg_reduce_desc desc{};
        bool planes = false;             // the planes, not the RGB24 frames
        dg_plane_reduce_desc pdesc{};
        int16_t *distance = nullptr;
        uint8_t *kind = nullptr;
        uint16_t *id = nullptr;
        uint8_t *cls = nullptr;
        dg_label_box *boxes = nullptr;   // filled from `raw` when the copy has finished (finish_readback)
        LabelRawBox *raw = nullptr;      // where the box rows land as the kernels left them: h_rawboxes, or memory of a synchronous call's own
    } copy;                              // the pending asynchronous one (issued again if the batch has to be redone)
    bool copy_pending = false;
    DevPtr<uint8_t> d_reduced;           // reduced readbacks: the kernel's output, allocated by the first one, grown when a later one needs more
    size_t reduced_cap = 0;
    PinnedPtr<LabelRawBox> h_rawboxes;   // reduced plane readbacks that ask for boxes: the box rows as the kernels left them, likewise
    size_t rawbox_cap = 0;               // (entries)
    PinnedPtr<uint8_t> h_lists;   // pinned staging
    DevPtr<uint8_t> d_lists;
    DevPtr<DevRSpan> d_rspans;
    DevPtr<uint8_t> d_fb;
    size_t lists_cap = 0;
    // label frames: owner tags parallel to the wall records of d_lists (staging + HBM, wall_cap_per_batch entries) — they do not exist
    // before the slot's first label submission
    PinnedPtr<uint32_t> h_owners;
    DevPtr<uint32_t> d_owners;
    // The buffers whose size is the uploaded scene's: dg_upload_scene drops them, the first submission that needs one allocates it.
    struct PerScene {
        DevPtr<LabelRawBox> d_boxes;     // label frames: the box table max_batch x box_mobjs
        size_t box_mobjs = 0;
        PinnedPtr<uint32_t> h_masks;     // map frames: the mask rows of the last submission that had any (staging + HBM, max_batch x
        DevPtr<uint32_t> d_masks;        // mask_words), kept for dg_replay_slot
        size_t mask_words = 0;
        // floor-textured map frames: the cells [max_batch][sectors] of the last such submission (staging + HBM) and the
        // sector rows [max_batch][ceil(sectors / 32)] dg_floor_seen_sectors builds from its mask rows
        PinnedPtr<FloorCell> h_floor_cells;
        DevPtr<FloorCell> d_floor_cells;
        DevPtr<uint32_t> d_floor_seen;
        // map frames with markers: the last such submission's shown rows [n][ceil(map objects / 32)], entry index [n + 1]
        // and sorted pose entries in one block (staging + HBM), there from the slot's first such submission on and grown when one needs more
        PinnedPtr<uint8_t> h_things;
        DevPtr<uint8_t> d_things;
        size_t things_cap = 0;
        // per-view map-object poses, sector heights (§8n) and sector flats (§8p) through the seg walk.  Unlike the others
        // these are taken at dg_upload_scene (upload_fs_scene), so that nothing is allocated on the submit path.
        RowBuffers<PoseRows> poses;
        RowBuffers<HeightRows> heights;
        RowBuffers<FlatRows> flats;
        // ... and the surfaces' sidedef table (slab_layout.h's SurfaceLayout), there exactly when `flats` is
        PinnedPtr<uint8_t> h_side_table;
        DevPtr<uint8_t> d_side_table;
        void drop() { *this = PerScene{}; }
    } per_scene;
    // What a map submission (front_end DG_FE_MAP*) leaves for its kernels and for dg_replay_slot besides d_lists (the arrow lines, then a
    // player-centred submission's views) and the mask rows above: written as a whole by every such submission.
    struct MapState {
        dg_ego_map ego{};                // DG_FE_MAP_EGO, DG_FE_MAP_FLOOR: scale and flags
        bool masked = false;             // the kernel reads the slot's mask rows (a player-centred submission may come without)
        bool built = false;              // the enqueue built the kind's per-scene table: ev_start .. ev_setup time that
        bool things = false;             // a *_things submission: the kernels with the things phase, reading the slot's things block
        size_t things_first = 0, things_entries = 0;   // ... where its entry index and its entries start in that block (the rows: at 0)
    } map;
    // last submission
    RasterParams P{};
    uint32_t max_spans = 0;
    uint64_t n_spans = 0, covered = 0, list_bytes = 0, n_walls = 0, n_planes = 0;
    int n_frames = 0;
    float host_ms = 0.0f;         // list generation + binning + packing of the last submission
    // Where that submission stands.  Each step is written once: describe() (-> prepared), enqueue_kernels (-> queued, or
    // -> empty when it fails), make_final (queued -> settled) and reset() (-> empty).
    enum class Phase {
        Empty,                    // no submission (n_frames == 0): a fresh slot, every slot after dg_upload_scene, one whose enqueue failed half way
        Prepared,                 // lists or records are resident and have not run since they were built
        Queued,                   // kernels are enqueued: nobody has waited for them or looked at the overflow flags
        Settled                   // they have finished, frames that overflowed a capacity are redone: the framebuffer is final, the records still there to replay
    } phase = Phase::Empty;
    bool has_run() const { return phase >= Phase::Queued; }                        // the timing events are this submission's
    bool unchecked() const { return phase == Phase::Queued && column_walk(); }     // its overflow flags still have to be looked at
    void reset() { phase = Phase::Empty; n_frames = 0; snap_scene = nullptr; from_views = false; }     // (nothing may be replayed or redone from what the slot holds)
    // device column walk (DG_FE_DEVICE)
    PinnedPtr<uint8_t> h_fe;                    // record slab: pinned staging
    DevPtr<uint8_t> d_fe;                       // ... and HBM
    DevPtr<uint32_t> d_fe_coloff;
    PinnedPtr<uint32_t> h_status;               // pinned host memory the walk's kernels write: [F] overflow flags, [F] spans per frame
    uint64_t *d_events = nullptr;               // sky event bits (fe_event_words), zeroed before every walk: inside d_flags' allocation
    size_t walk_state_bytes = 0;                // that whole allocation (dg_create)
    bool walk_state_clean = false;              // d_flags .. is all zero (dg_fe_scan cleans up after the walk; enqueue_kernels clears a slot that is not)
    DevPtr<uint32_t> d_order;                   // dg_fe_columns' launch-order lists as dg_fs_frame builds them (FsParams::order_list)
    DevPtr<uint32_t> d_flags;                   // [F] overflow flags the walk's kernels OR into; sits in front of d_events (one memset clears both)
    FeParams FP{};
    FsParams FSP{};               // DG_FE_DEVICE_SEGS: the device seg walk in front of the column walk
    LfxRows LR{};                 // ... and, with the light effects on, dg_light_rows in front of it (LR.n_frames 0: not launched)
    MfxRows MR{};                 // ... and, with the map-object thinkers on, dg_mobj_rows (MR.n_frames 0: not launched)
    RowRun<PoseRows> pose_run;    // ... and, for a batch with poses, dg_mobj_pose_fill / _place in front of them all
    RowRun<HeightRows> height_run;   // ... and, for a batch with sector entries or surfaces, dg_sector_row_fill / _scatter; the seg walk is then the row-reading pair
    RowRun<FlatRows> flat_run;    // ... and, for a batch with surfaces, dg_flat_row_fill / _scatter behind them; the seg walk is then the dg_sfc_* pair, given SF
    FsSurf SF{};
    // What the last submission went through, as dg_timing.front_end reports it: DG_FE_HOST, DG_FE_DEVICE (the device column walk),
    // DG_FE_DEVICE_SEGS (... with the per-seg half on the GPU too), DG_FE_MAP / DG_FE_MAP_EXPLORED / DG_FE_MAP_EGO (2-D map frames: arrow lines at the start of d_lists) or
    // DG_FE_DEPTH (host lists walked by dg_depth_tiles: the framebuffer slab holds the two planes, not RGB24) or DG_FE_LABELS (host lists
    // walked by dg_label_tiles: the slab holds the id and class planes) or DG_FE_BUNDLE (host lists run through the colour kernels and / or
    // dg_bundle_tiles: the slab holds the parts bundle_what names, laid out by bundle_layout)
    int32_t front_end = DG_FE_HOST;
    uint32_t bundle_what = 0;     // DG_BUNDLE_* of the last submission when it was a bundle
    // A new submission of n frames through front end fe, `bytes` of lists or records uploaded for it (span statistics: the host list path's alone)
    void describe(int32_t fe, int n, uint64_t bytes, uint64_t walls, uint64_t planes) {
        front_end = fe; phase = Phase::Prepared; n_frames = n; list_bytes = bytes; n_walls = walls; n_planes = planes;
        max_spans = 0; n_spans = 0; covered = 0;
    }
    bool column_walk() const { return front_end == DG_FE_DEVICE || front_end == DG_FE_DEVICE_SEGS; }
    bool seg_walk() const { return front_end == DG_FE_DEVICE_SEGS; }
    bool map_frames() const { return front_end == DG_FE_MAP || front_end == DG_FE_MAP_EXPLORED || front_end == DG_FE_MAP_EGO || front_end == DG_FE_MAP_FLOOR; }   // arrow lines at the start of d_lists
    // This submission has a timed front half (ev_start .. ev_setup): a depth or label submission has none, a map submission only when it
    // built its kind's per-scene table.
    bool timed_front_half() const { return front_end != DG_FE_DEPTH && front_end != DG_FE_LABELS && (!map_frames() || map.built); }
    bool holds_bundle() const { return front_end == DG_FE_BUNDLE && phase != Phase::Empty; }
    // Which parts the framebuffer slab holds (BUNDLE_*: RGB24 colour frames, the two depth planes, the two label planes) ...
    uint32_t parts() const {
        if (phase == Phase::Empty) return 0;
        if (front_end == DG_FE_BUNDLE) return bundle_what;
        return front_end == DG_FE_DEPTH ? BUNDLE_DEPTH : front_end == DG_FE_LABELS ? BUNDLE_LABELS : BUNDLE_COLOUR;
    }
    bool holds(uint32_t part) const { return (parts() & part) != 0; }
    // ... and where each sits.  A bundle's parts are where bundle_layout puts them, each on the slab's boundary; the one part of any
    // other submission starts at the slab's base, its 8-bit plane right behind its 16-bit plane (include/doomgpu.h promises 2 n W H).
    BundleLayout layout(size_t W, size_t H) const {
        if (front_end == DG_FE_BUNDLE) return bundle_layout((size_t)n_frames, W, H, bundle_what);
        const size_t px = (size_t)n_frames * W * H;
        return BundleLayout{0, 0, 2 * px, 0, 2 * px, 3 * px};
    }
    bool harvested = true;        // DG_FE_AUTO has read this submission's GPU time
    std::vector<dg_view> views;   // the views of that submission (to redo it on the host if a capacity overflowed)
    // ... and a private copy of what they brought (KeptInputs), taken by built_from and by nothing else — no builder
    // writes it, because redo_overflowed hands it to one.  A frame redone on the host is drawn with it, and dg_slot_mobj_poses /
    // _sector_heights / _sector_flats derive the rows of a host-walker submission from it.  from_views: the slot's submission was built
    // from views (not from the caller's lists, not a 2-D map submission) — the submit functions say so once it is built.
    KeptInputs kept;
    bool from_views = false;
    // The scene's own light levels and map-object states as they were when the batch was submitted: a frame that overflows a capacity is
    // redone at dg_wait time from the host walker, and dg_scene_set_sector_light / _mobj_state may have moved the scene on by then
    // (lights.rs:47-259 and map_objects.rs:63-121 run between two submissions of a pipelined caller).
    const Scene *snap_scene = nullptr;
    uint64_t snap_rev = 0;
    std::vector<dg_sector_light> snap_lights;
    std::vector<dg_mobj_state> snap_mobjs;
    void snapshot_scene(const Scene &sc) {
        if (snap_scene == &sc && snap_rev == sc.revision && snap_lights.size() == sc.sectors.size() && snap_mobjs.size() == sc.mobjs.size()) return;
        snap_lights.resize(sc.sectors.size()); snap_mobjs.resize(sc.mobjs.size());
        for (size_t i = 0; i < sc.sectors.size(); i++) snap_lights[i] = dg_sector_light{(int32_t)i, (int32_t)sc.sectors[i].light};
        for (size_t i = 0; i < sc.mobjs.size(); i++) snap_mobjs[i] = dg_mobj_state{(int32_t)i, sc.mobjs[i].sprite_frame, sc.mobjs[i].full_bright ? 1 : 0, 0};
        snap_scene = &sc; snap_rev = sc.revision;
    }
    // The game state frame i of the last submission was rendered with, for the host walker: nullptr = the scene as it is (unchanged since the
    // submission, no per-view snapshot); else the submit-time scene state with the view's own entries on top (later entries win).
    struct RedoState { std::vector<dg_sector_light> lights; std::vector<dg_mobj_state> mobjs; dg_view_state st{}; };
    // fx: the effects the frame was drawn with — the light effects' sectors keep the effect's level and the objects the thinkers drive
    // their state, so the snapshot does not list them.
    const dg_view_state *state_for_redo(const Scene &sc, int i, RedoState &tmp, const SceneFx &fx) const {
        const dg_view_state *own = kept.at(i).state;
        if (snap_scene != &sc || snap_rev == sc.revision) return own;
        tmp.lights.clear();
        const bool lfx = fx.light.fits(sc), mfx = fx.mobj.fits(sc);      // (the snapshot has the scene's sizes: snapshot_scene)
        for (const dg_sector_light &l : snap_lights)
            if (!lfx || fx.light.rec_of[(size_t)l.sector] < 0) tmp.lights.push_back(l);
        tmp.mobjs.clear();
        for (const dg_mobj_state &m : snap_mobjs)
            if (!mfx || fx.mobj.type_of[(size_t)m.mobj] < 0) tmp.mobjs.push_back(m);
        if (own) { tmp.lights.insert(tmp.lights.end(), own->lights, own->lights + own->n_lights); tmp.mobjs.insert(tmp.mobjs.end(), own->mobjs, own->mobjs + own->n_mobjs); }
        tmp.st = dg_view_state{tmp.lights.data(), (uint32_t)tmp.lights.size(), tmp.mobjs.data(), (uint32_t)tmp.mobjs.size()};
        return &tmp.st;
    }
};

static_assert(std::is_move_constructible_v<Slot> && !std::is_copy_constructible_v<Slot>, "dg_ctx::slots (a std::vector, resized at dg_create) moves its slots");

struct FeFrameOut {               // parts-mode output of one frame, owned per batch index
    std::vector<FePart> parts;
    std::vector<FeSprite> sprites;
    std::vector<uint32_t> behind, sky_parts, bin_off, sbin_off;
    std::vector<uint16_t> bin_parts, sbin_sprites;
    uint32_t behind_words = 0, n_sky_slots = 0;
    DevFrame hdr{};
};

}  // namespace dg

using namespace dg;                    // (as the files that include this do)

struct dg_ctx {
    dg_config cfg{};
    FrameConsts fk{};
    DevConsts dk{};
    const Scene *scene = nullptr;
    size_t uploaded_flats = 0, uploaded_anims = 0;   // flat pool size and animation lists at dg_upload_scene time (dg_scene_use_flat adds to both)
    size_t uploaded_texels = 0;         // texel pool size at dg_upload_scene time (grows when new sprite bitmaps are decoded)
    // device scene
    DevPtr<uint32_t> d_palette;         // 256 x u32 RGBX, followed by 256 x (r, g, b, 0) f32
    DevPtr<uint8_t> d_texel_idx, d_texel_opq;
    uint8_t *d_flats = nullptr;         // inside d_texel_idx's allocation
    DevPtr<unsigned long long> d_checksums;      // dg_frame_checksums scratch, max_batch entries
    DevPtr<uint4> d_row_tab;            // per-row constants of the flat / sky mappers (dg_row_table), rebuilt per scene upload
    DevScene dscene{};
    std::vector<Slot> slots;
    Stream kstream;                     // every kernel of every slot, in submission order (enqueue_kernels)
    Stream rstream;                     // raster_overlap: the raster launches, so that the next batch's front-end kernels (kstream) run next to them
    bool raster_overlap = false;
    std::unique_ptr<Pool> pool;
    std::vector<std::unique_ptr<FrameArena>> arenas;   // one per worker (+ caller)
    std::vector<BinnedFrame> binned;                   // one per frame of a batch
    std::vector<std::vector<uint32_t>> label_tags;     // label submissions: the owner tag of every wall record of binned[i]
    size_t span_cap_per_batch = 0, wall_cap_per_batch = 0, plane_cap_per_batch = 0;
    int n_threads = 1;
    // device column walk
    bool fe_enabled = false;            // cfg.front_end asks for it
    bool fe_scene_ok = false;           // ... and the uploaded scene allows it (sky bitmap >= 256x128, see bin_frame)
    // device seg walk (DG_FE_DEVICE_SEGS): the scene's per-seg tables + BSP tables in one allocation, per-batch scratch sized by the scene
    bool fs_enabled = false, fs_scene_ok = false;
    bool fs_rows_dirty = true;          // the seg walk's candidate rows may hold entries (fresh allocation, or a launch that failed half way)
    bool preparing = false;             // inside dg_prepare_views: the records are built once and replayed — host time is not in the loop
    bool fs_forced = false;             // DG_FE_DEVICE_SEGS: always; DG_FE_AUTO: when it is the faster way for the batch at hand (choose_fs)
    FeAuto fe_auto;                     // what DG_FE_AUTO has measured and decides by
    DevPtr<uint8_t> d_fs_scene;
    // the scene's effects as of dg_upload_scene (every front end draws with this copy), and for the seg walk the device tables of each
    // effect that is on (only while the seg walk is uploaded)
    SceneFx fx;
    std::vector<dg_map_marker> markers; // ... and its marker table (dg_scene_set_map_markers), or empty
    DevPtr<uint8_t> d_wall_fx;          // FsSegFx per seg | the live animation lists
    FsFx fs_fx{};
    DevPtr<uint8_t> d_light_fx;         // LfxRec per effect sector | rec_of per sector | tables
    LfxRows lfx_proto{};                // its pointers and the seed, filled at upload
    DevPtr<uint8_t> d_mobj_fx;          // steps | chains | types | type_of per map object | events
    MfxRows mfx_proto{};                // its pointers and counts, filled at upload
    DevPtr<uint8_t> d_fs_scratch;       // occupancy rows (zero between batches) | candidate rows F x n_segs x 5 x 8 B | candidate lists + keep bits of frames beyond FS_CL_CAP
    size_t fs_zero_bytes = 0;
    FsParams fs_proto{};                // scene pointers and counts, filled at upload
    const int32_t *d_seg_side = nullptr;          // every seg's front sidedef, in d_fs_scene: what a frame's sidedef entries are searched by
    // the row kernels' scene side, in d_fs_scene, filled at upload: the table as loaded that the rows start as, its length, and the pose
    // kernels' BSP and leaf sectors (scene_rows null: the scene has no such rows)
    PoseParams pose_proto{};
    SectorRowParams height_proto{};
    FlatRowParams flat_proto{};
    uint64_t fallbacks_fe = 0;          // batches in which frames were redone because a device-side capacity was exceeded (dg_ctx_fallbacks)
    uint64_t redone_frames = 0;         // frames redone through the host list path, one at a time (dg_ctx_redone_frames)
    DevPtr<DevRSpan> d_redo_rspans;     // resolved spans of ONE frame being redone (allocated on first use)
    size_t redo_span_cap = 0;
    std::vector<FeFrameOut> fe_out;     // one per frame of a batch
    uint32_t fe_col_slots = FE_DEFAULT_COL_SLOTS;
    size_t fe_part_cap = 0, fe_sprite_cap = 0, fe_behind_cap = 0, fe_bin_cap = 0, fe_sbin_cap = 0, fe_slab_cap = 0;
    DevPtr<uint32_t> d_fe_cnt;
    DevPtr<FeU4> d_fe_cspans;
    DevPtr<FeColRec> d_fe_recs;
    // Device tables derived from the uploaded scene.  Each is made by the first call that needs it after dg_upload_scene, which drops
    // them all: a table is valid exactly when its pointer is set (each is assigned only once it is complete).
    struct PerScene {
        DevPtr<uint8_t> map_layer;          // 2-D map view: every drawn linedef at the ctx's frame size, RGB24 (build_map_layer)
        DevPtr<uint32_t> cover, chains;     // explored-map frames: explored_core.h's cover and its chains (upload_explored_cover)
        DevPtr<uint8_t> ego_table;          // player-centred map frames: EgoLine per linedef, then a word per linedef (upload_ego_table)
        uint32_t ego_lines = 0;
        DevPtr<uint8_t> floor_table;        // floor-textured map frames: segs, nodes, leaves and the linedefs' sectors (upload_floor_table)
        FloorTables floor_T{};              // ... as dg_floor_map_tiles reads them
        const FloorLine *floor_lines = nullptr;
        DevPtr<uint8_t> thing_table;        // map frames with markers: ThingMarker per map object, then ThingPlace per map object (upload_thing_table)
        uint32_t things = 0;                // ... their count; 0 with a table: the ctx took no marker table
        DevPtr<uint32_t> seg_line;          // dg_seen_lines_device / dg_slot_seen_lines: seg -> linedef (ensure_seen)
        DevPtr<uint32_t> seen_scratch;      // dg_slot_seen_lines: its scratch rows, sized by max_batch and the scene's row length
        DevPtr<uint8_t> walk_tables;        // dg_ctx_locate_walks: the node and leaf tables (walk_core.h)
        const WalkNode *walk_nodes = nullptr;
        const WalkLeaf *walk_leaves = nullptr;
        // dg_sight_device / dg_sight_mobjs_device: the scene's sight tables, its map objects, leaf sectors and one height
        // row in one allocation (ensure_sight); the rows [max_batch][sectors] and [max_batch][map objects] of a call with entries; and
        // one block for a call's entries, inputs and results, grown when a call needs more
        DevPtr<uint8_t> sight_table;
        SightTables sight_T{};              // ... as the kernels read them, over the scene's one row
        const FsMobj *sight_mobjs = nullptr;
        const int32_t *sight_leaf_sector = nullptr;
        uint32_t sight_depth = 0;           // the BSP's depth (sight_core.h sight_depth)
        DevPtr<FsHeights> sight_rows;
        DevPtr<FsMobj> sight_poses;
        DevPtr<uint8_t> sight_io;
        size_t sight_io_cap = 0;
        void drop() { *this = PerScene{}; }
    } per_scene;
    Stream wstream;                     // dg_ctx_locate_walks: a stream of its own, created by the first call — the slots' streams and the kernel stream are not touched
    // dg_reduce_device: likewise a stream of its own and the events attached to its last call's kernel, created by the first call
    Stream xstream;
    TimedInterval reduce;
    TimedInterval plane_reduce;         // dg_reduce_planes_device: the same stream, events of its own
    TimedInterval observe;              // dg_observe_device: likewise
    TimedInterval seen, seen_acc;       // dg_seen_lines_device / dg_slot_seen_lines: the events of the last call's kernels, on xstream
    TimedInterval sight_rows, sight;    // dg_sight_device / dg_sight_mobjs_device: the last call's row kernels (unmeasured without entries) and its sight kernel, on xstream
    // dg_overlay_device / dg_slot_overlay: the scene's screen pictures as of dg_upload_scene (a handle beyond them was loaded since), the
    // device scratch a call stages its item and rectangle records in (grown when a call needs more), and the last call's kernel, on xstream
    std::vector<OvlPicture> pictures;
    DevPtr<uint8_t> d_overlay;
    size_t overlay_cap = 0;
    TimedInterval overlay;

    // The members' owners free the memory, the streams and the events: with the ctx's device current, and only after every stream that
    // may still use them has drained.  (A ctx whose creation failed half way comes here with some of them still empty.)
    ~dg_ctx() {
        (void)hipSetDevice(cfg.device);
        drain(kstream);                 // every slot's kernels, before anything they use is freed
        drain(rstream);
        for (Slot &s : slots) { drain(s.stream); drain(s.copy_stream); }
        drain(wstream);
        drain(xstream);
    }
};

namespace dg {

// Everything queued for the slot so far has finished (its kernels run on the ctx's kernel stream, the rest on its own).
hipError_t slot_sync(Slot &s);
int check_slot(dg_ctx *c, int slot);
enum class Copy { Leave, Complete };                   // what make_final does about the slot's pending dg_readback_async
int make_final(dg_ctx *c, Slot &s, Copy copy);
// api_readback.cpp's, for make_final and dg_upload_scene: the slot's pending readback queued on its copy stream behind its kernels, and
// what is left to do on the host once a readback's copies have finished; for dg_replay_slot: a slot without a colour part is refused.
int enqueue_copy(dg_ctx *c, Slot &s);
void finish_readback(const dg_ctx *c, const Slot &s, const Slot::Readback &r);
int refuse_no_colour(const Slot &s, const char *what);

// What the reduced readbacks and dg_reduce_device check before anything else.
inline int check_reduce_desc(const dg_reduce_desc *desc) {
    if (!desc) return set_err(DG_ERR_INVALID, "null argument");
    if (!reduce_desc_ok(*desc)) return set_err(DG_ERR_INVALID, "reduce descriptor: fx and fy in 1..16, a known format, reserved 0");
    return DG_OK;
}

}  // namespace dg
