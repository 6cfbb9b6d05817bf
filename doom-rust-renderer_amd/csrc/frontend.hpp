// frontend.hpp — per-frame list generation on the host.
//
// The reference draws solid walls inline while it walks the BSP and records a replay list for masked walls
// and sprites (src/renderer/segs.rs:185-200,231-260,349).  Here the same walk records *everything* — no
// pixel is touched on the host — and emits the lists in the order the reference would have drawn them:
//   1. solid / upper / lower wall records, BSP front-to-back           (src/renderer/mod.rs:61-104)
//   2. visplanes in push order                                          (src/renderer/mod.rs:106-116)
//   3. sprites far->near, each preceded by the masked walls behind it  (src/renderer/map_objects.rs:216-240)
//   4. remaining masked walls                                           (src/renderer/segs.rs:593-597)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <algorithm>

#include "../../include/doomgpu.h"
#include "fe_dev.h"
#include "scene.hpp"
#include "view_rows_core.h"

namespace dg {

// A view's entries for the items of one scene table as they stand: of two entries for one index the later wins, at the place of the
// first.  Index: the entry's member that names its item.  begin(n) starts a view over n items (the one before has been released),
// put(value) takes an entry whose index has been checked, release() hands the index row back all -1 and leaves out as it is, in any
// order — O(entries), so that an arena's row is never cleared whole.
template <class T, int32_t T::*Index> struct LatestPerIndex {
    std::vector<int32_t> of;        // per item: its entry in out, or -1
    std::vector<T> out;             // one entry per item that has any, in the order of the items' first entries
    void begin(size_t n_items) {
        out.clear();
        if (of.size() != n_items) of.assign(n_items, -1);
    }
    __attribute__((always_inline)) void put(const T &value) {        // (once per entry of a batch — millions: never a call of its own)
        int32_t &at = of[(size_t)(value.*Index)];
        if (at < 0) { at = (int32_t)out.size(); out.push_back(value); }
        else out[(size_t)at] = value;
    }
    void release() {
        for (const T &value : out) of[(size_t)(value.*Index)] = -1;
    }
};
using LatestPoses = LatestPerIndex<dg_mobj_pose, &dg_mobj_pose::mobj>;
using LatestHeights = LatestPerIndex<dg_sector_heights, &dg_sector_heights::sector>;
using LatestSides = LatestPerIndex<FsSideEntry, &FsSideEntry::sidedef>;
using LatestFlats = LatestPerIndex<FlatEntry, &FlatEntry::sector>;

struct FrameConsts {   // src/renderer/constants.rs:3-17, evaluated in f32 exactly like the const items
    float ARC, GSW, GCFX, CFX, CFY;
    int W, H;
};
FrameConsts make_consts(int W, int H);

// Reusable per-thread storage: one build() call fills it, the dg_frame_lists view points into it.
struct FrameArena {
    std::vector<dg_bitmap_render> renders;
    std::vector<uint32_t> owners;       // per render: the owner tag of the seg or map object that made it (doomgpu.h: dg_build_lists_owners)
    std::vector<dg_bitmap_column> columns;
    std::vector<dg_visplane> visplanes;
    std::vector<int16_t> plane_tb;
    std::vector<dg_draw_cmd> order;
    // parts mode (device column walk): per-seg / per-sprite records instead of finished columns
    std::vector<FePart> parts;
    std::vector<FeSprite> sprites;
    std::vector<uint32_t> sky_parts;    // per sky slot: index of the part
    std::vector<uint32_t> bin_off, sbin_off;         // column bins (fe_dev.h): n_bins + 1 offsets each
    std::vector<uint16_t> bin_parts, sbin_sprites;
    std::vector<uint32_t> behind;       // n_sprites rows of behind_words bits: wall record p is behind sprite s
    uint32_t behind_words = 0, n_sky_slots = 0;
    // scratch
    struct Rec;
    std::vector<Rec> *recs = nullptr;   // opaque (defined in frontend.cpp)
    std::vector<int16_t> floor_tb, ceil_tb;
    std::vector<uint8_t> hor_ocl;
    std::vector<int16_t> floor_ocl, ceil_ocl, top_clip, bottom_clip;
    // per sector / per map object: the value this view draws with (its snapshot entry, else the effect's value at its tics) or "no
    // override"; the Walker writes the entries of one frame and takes them back
    std::vector<int32_t> light_row, mobj_row;
    // the view's poses (per map object), sector entries (per sector) and surface entries (per sidedef / per sector) as they stand
    // (resolve_view_*); written and taken back likewise
    LatestPoses poses;
    LatestHeights heights;
    LatestSides sides;
    LatestFlats flats;
    // the heights / flats one view is drawn with, [sector] — the scene's with those entries on top, written whole by every Walker that has entries
    std::vector<FsHeights> height_row;
    std::vector<FsFlats> flat_row;
    FrameArena();
    ~FrameArena();
    FrameArena(const FrameArena &) = delete;
    FrameArena &operator=(const FrameArena &) = delete;
};

// What one view may bring besides the view itself (include/doomgpu.h); each is optional.  A further per-view input is one member
// here, in BatchInputs and in KeptInputs, one line in check_view_inputs, and its consumer.
struct ViewInputs {
    const dg_view_state *state = nullptr;         // the view's game-state snapshot (dg_view_state); nullptr: the scene's state
    const dg_view_poses *poses = nullptr;         // where the view's map objects are (dg_view_poses); nullptr: where the scene has them
    const dg_view_sectors *sectors = nullptr;     // the view's sector floor / ceiling heights (dg_view_sectors); nullptr: as loaded
    const dg_view_surfaces *surfaces = nullptr;   // the view's sidedef textures and offsets and sector flats (dg_view_surfaces); nullptr: as loaded
    ViewInputs() = default;
    // (not explicit: a caller with a state alone, or none — nullptr — passes it as before)
    ViewInputs(const dg_view_state *st, const dg_view_poses *ps = nullptr, const dg_view_sectors *vs = nullptr, const dg_view_surfaces *vf = nullptr)
        : state(st), poses(ps), sectors(vs), surfaces(vf) {}
    bool any() const { return state || poses || sectors || surfaces; }
};
// ... and a batch's: each null, or one element per view.
struct BatchInputs {
    const dg_view_state *states = nullptr;
    const dg_view_poses *poses = nullptr;
    const dg_view_sectors *sectors = nullptr;
    const dg_view_surfaces *surfaces = nullptr;
    bool any() const { return states || poses || sectors || surfaces; }
    __attribute__((always_inline)) ViewInputs at(int i) const {     // (once per frame, inside the builders' per-frame lambdas)
        return ViewInputs{states ? states + i : nullptr, poses ? poses + i : nullptr, sectors ? sectors + i : nullptr, surfaces ? surfaces + i : nullptr};
    }
};

// A private copy of a batch's inputs, entries included: the caller's arrays need not outlive the call that handed them over.  Every
// view's entries of one kind lie in one flat vector, and the per-view structs point into it.
class KeptInputs {
    std::vector<dg_view_state> states;
    std::vector<dg_sector_light> lights;
    std::vector<dg_mobj_state> mobjs;
    std::vector<dg_view_poses> poses;
    std::vector<dg_mobj_pose> pose_entries;
    std::vector<dg_view_sectors> sectors;
    std::vector<dg_sector_heights> height_entries;
    std::vector<dg_view_surfaces> surfaces;
    std::vector<dg_side_surface> side_entries;
    std::vector<dg_sector_flats> flat_entries;
    // views: the caller's structs of one kind, copied as they are; the arrays they name through (ptr, count) go into `flat` one after
    // the other, and only then — the vector has stopped growing — are the copies pointed at their part of it.  An array may be null
    // when its count is 0.
    template <class V, class E> static void flatten(std::vector<V> &views, std::vector<E> &flat, const E *V::*ptr, uint32_t V::*count) {
        flat.clear();
        for (const V &v : views)
            if (v.*count) flat.insert(flat.end(), v.*ptr, v.*ptr + v.*count);
        size_t at = 0;
        for (V &v : views) { v.*ptr = flat.data() + at; at += v.*count; }
    }
    template <class V> static void copy_views(std::vector<V> &views, const V *from, int n) {
        if (from) views.assign(from, from + n);
        else views.clear();
    }

public:
    // A deep copy of n views' inputs (checked: check_view_inputs) in place of what was kept; an empty `in` keeps nothing.
    void keep(const BatchInputs &in, int n) {
        copy_views(states, in.states, n); copy_views(poses, in.poses, n); copy_views(sectors, in.sectors, n); copy_views(surfaces, in.surfaces, n);
        flatten(states, lights, &dg_view_state::lights, &dg_view_state::n_lights);
        flatten(states, mobjs, &dg_view_state::mobjs, &dg_view_state::n_mobjs);
        flatten(poses, pose_entries, &dg_view_poses::poses, &dg_view_poses::n);
        flatten(sectors, height_entries, &dg_view_sectors::heights, &dg_view_sectors::n);
        flatten(surfaces, side_entries, &dg_view_surfaces::sides, &dg_view_surfaces::n_sides);
        flatten(surfaces, flat_entries, &dg_view_surfaces::flats, &dg_view_surfaces::n_flats);
    }
    // What is kept, pointing into this object until its next keep(): null for every input that was not given.
    BatchInputs inputs() const {
        return BatchInputs{states.empty() ? nullptr : states.data(), poses.empty() ? nullptr : poses.data(), sectors.empty() ? nullptr : sectors.data(),
                           surfaces.empty() ? nullptr : surfaces.data()};
    }
    ViewInputs at(int i) const { return inputs().at(i); }
};

// Fills `arena` and `out` (pointers into arena).  Returns DG_OK or DG_ERR_RENDER with `err` set where the
// reference would panic.  `view` must have its trig fields filled.
// `fx` (optional): the effects to draw with (Scene::fx, or the copy a dg_ctx uploaded); nullptr: none.
int build_frame_lists(const Scene &sc, int W, int H, const dg_view &view, FrameArena &arena, dg_frame_lists &out, std::string &err,
                      const ViewInputs &in = {}, const SceneFx *fx = nullptr);

// Checks a view's snapshot against the scene's ranges and hands every valid entry, in order (later entries win), to light(sector, level)
// or mobj(map object, mfx_encode'd state).  Returns 0, or bit 0: a sector index was out of range, bit 1: a map object or sprite frame
// index was.  The host walker and build_batch_fs (context.cpp) both go through it.
template <class LightFn, class MobjFn>
unsigned apply_view_state(const Scene &sc, const dg_view_state &st, LightFn light, MobjFn mobj) {
    unsigned bad = 0;
    for (uint32_t i = 0; i < st.n_lights; i++) {
        const dg_sector_light &l = st.lights[i];
        if (l.sector < 0 || (size_t)l.sector >= sc.sectors.size()) bad |= 1u;
        else light((size_t)l.sector, l.light_level);
    }
    for (uint32_t i = 0; i < st.n_mobjs; i++) {
        const dg_mobj_state &m = st.mobjs[i];
        if (m.mobj < 0 || (size_t)m.mobj >= sc.mobjs.size() || m.sprite_frame >= (int32_t)sc.sprite_frames.size()) bad |= 2u;
        else mobj((size_t)m.mobj, mfx_encode(m.sprite_frame, m.full_bright));
    }
    return bad;
}

// A view's poses as they stand: every entry is checked against the scene's range, and of two entries for one object the later wins.
// poses.out: one entry per moved object, in the order of the objects' first entries; poses.of[object]: its place there, else -1,
// until the caller's poses.release().  Returns false when an object index was out of range (the entries that are in range still
// stand).  The host walker, build_batch_fs (context.cpp) and dg_slot_mobj_poses all go through it.
inline bool resolve_view_poses(const Scene &sc, const dg_view_poses &vp, LatestPoses &poses) {
    poses.begin(sc.mobjs.size());
    bool ok = true;
    for (uint32_t i = 0; i < vp.n; i++) {
        const dg_mobj_pose &p = vp.poses[i];
        if (p.mobj < 0 || (size_t)p.mobj >= sc.mobjs.size()) { ok = false; continue; }
        poses.put(p);
    }
    return ok;
}

// A view's sector heights as they stand, by the same rules: of two entries for one sector the later wins; heights.out holds one entry
// per sector in the order of the sectors' first entries, heights.of[sector] its place there, else -1, until the caller's
// heights.release().  Returns 0, or bit 0: a sector index out of range, bit 1: a height outside int16 (the other entries still
// stand).  The host walker, build_batch_fs (context.cpp) and dg_slot_sector_heights all go through it.
inline unsigned resolve_view_sectors(const Scene &sc, const dg_view_sectors &vs, LatestHeights &heights) {
    heights.begin(sc.sectors.size());
    unsigned bad = 0;
    for (uint32_t i = 0; i < vs.n; i++) {
        const dg_sector_heights &h = vs.heights[i];
        if (h.sector < 0 || (size_t)h.sector >= sc.sectors.size()) { bad |= 1u; continue; }
        if (h.floor_height < -32768 || h.floor_height > 32767 || h.ceiling_height < -32768 || h.ceiling_height > 32767) { bad |= 2u; continue; }
        heights.put(h);
    }
    return bad;
}
inline const char *view_sectors_error(unsigned bad) {
    return bad & 1u ? "view sectors: sector index out of range" : "view sectors: height outside int16";
}

// A view's surfaces as they stand, by the same rules: of two entries for one sidedef or one sector the later wins.  sides holds one
// FsSideEntry per sidedef, sorted by sidedef — the span fs_side_find searches — each texture with the live wall animation list it
// belongs to (wall: the effects drawn with, or nullptr); flats one FlatEntry per sector, sorted by sector, tagged with `frame`.
// Both are released here (sides.of / flats.of all -1 before and after): the callers read sides.out and flats.out alone.  Returns 0, or
// bit 0: a sidedef index out of range, bit 1: a texture id that is neither DG_TEX_NONE nor a wall texture of the scene, bit 2: an offset
// outside int16, bit 3: a sector index out of range, bit 4: a flat handle not of this scene, bit 5: a null array with n > 0 (the other
// entries still stand).  The host walker, build_batch_fs (context.cpp) and dg_slot_sector_flats all go through it.
inline unsigned resolve_view_surfaces(const Scene &sc, const WallFx *wall, const dg_view_surfaces &vs, int32_t frame, LatestSides &sides,
                                      LatestFlats &flats) {
    sides.begin(sc.sidedefs.size());
    flats.begin(sc.sectors.size());
    unsigned bad = 0;
    if ((vs.n_sides && !vs.sides) || (vs.n_flats && !vs.flats)) return 32u;
    const auto list_of = [&](int32_t tex) -> int8_t {
        if (wall && tex >= 0)
            for (size_t l = 0; l < wall->lists.size(); l++)
                for (int k = 0; k < wall->lists[l].n; k++)
                    if (wall->lists[l].flat[k] == tex) return (int8_t)l;
        return (int8_t)-1;
    };
    for (uint32_t i = 0; i < vs.n_sides; i++) {
        const dg_side_surface &e = vs.sides[i];
        if (e.sidedef < 0 || (size_t)e.sidedef >= sc.sidedefs.size()) { bad |= 1u; continue; }
        bool tex_ok = true;
        for (int32_t t : {e.tex_mid, e.tex_low, e.tex_up}) tex_ok &= t == DG_TEX_NONE || sc.is_wall_texture(t);
        if (!tex_ok) { bad |= 2u; continue; }
        if (e.x_offset < -32768 || e.x_offset > 32767 || e.y_offset < -32768 || e.y_offset > 32767) { bad |= 4u; continue; }
        const FsSideEntry en{e.sidedef, e.tex_mid, e.tex_low, e.tex_up, list_of(e.tex_mid), list_of(e.tex_low), list_of(e.tex_up), 0, (int16_t)e.x_offset, (int16_t)e.y_offset};
        sides.put(en);
    }
    for (uint32_t i = 0; i < vs.n_flats; i++) {
        const dg_sector_flats &e = vs.flats[i];
        if (e.sector < 0 || (size_t)e.sector >= sc.sectors.size()) { bad |= 8u; continue; }
        if (!sc.is_flat_handle(e.floor_flat) || !sc.is_flat_handle(e.ceil_flat)) { bad |= 16u; continue; }
        flats.put(FlatEntry{frame, e.sector, FsFlats{e.floor_flat, e.ceil_flat}});
    }
    sides.release();
    flats.release();
    std::sort(sides.out.begin(), sides.out.end(), [](const FsSideEntry &a, const FsSideEntry &b) { return a.sidedef < b.sidedef; });
    std::sort(flats.out.begin(), flats.out.end(), [](const FlatEntry &a, const FlatEntry &b) { return a.sector < b.sector; });
    return bad;
}
inline const char *view_surfaces_error(unsigned bad) {
    return bad & 32u ? "view surfaces with a null array" : bad & 1u ? "view surfaces: sidedef index out of range" : bad & 2u ? "view surfaces: not a wall texture id of this scene"
         : bad & 4u ? "view surfaces: offset outside int16" : bad & 8u ? "view surfaces: sector index out of range" : "view surfaces: not a flat handle of this scene";
}

// The one rule every entry point checks before anything reads a view's inputs: no array is null with a count above 0.  False, with
// `why` set, otherwise.
inline bool check_view_inputs(const ViewInputs &in, std::string &why) {
    const char *bad = nullptr;
    if (in.state && ((in.state->n_lights && !in.state->lights) || (in.state->n_mobjs && !in.state->mobjs))) bad = "view state with a null array";
    else if (in.poses && in.poses->n && !in.poses->poses) bad = "view poses with a null array";
    else if (in.sectors && in.sectors->n && !in.sectors->heights) bad = "view sectors with a null array";
    else if (in.surfaces && ((in.surfaces->n_sides && !in.surfaces->sides) || (in.surfaces->n_flats && !in.surfaces->flats))) bad = view_surfaces_error(32u);
    if (bad) why = bad;
    return !bad;
}

void fill_view_trig(dg_view &v);

// Parts mode: the per-seg and per-sprite half only (BSP order, transform, clip, projection, pegging, sprite sorting and the
// sprite / masked-wall draw sequence); fills arena.parts / sprites / behind.  The per-column half runs on the GPU (frontend.hip).
// Returns DG_OK, DG_ERR_RENDER (the reference would panic before any column is walked) or kPartsUnsupported (a case only the
// host list path can judge: the caller redoes the frame with build_frame_lists).
constexpr int kPartsUnsupported = 1000;
int build_frame_parts(const Scene &sc, int W, int H, const dg_view &view, FrameArena &arena, std::string &err, const ViewInputs &in = {},
                      const SceneFx *fx = nullptr);

// Per-record constants of render_vertical_bitmap_line (bitmap_render.rs:233-251), shared by the binner and the parts builder.
DevWallRec make_wall_rec(const BitmapInfo &bi, float lsx, float lsy, float lex, float ley, float start_offset, int32_t start_x, int32_t end_x,
                         float bottom_height, float top_height, int16_t offset_x, int16_t offset_y, int16_t light_level);

}  // namespace dg
