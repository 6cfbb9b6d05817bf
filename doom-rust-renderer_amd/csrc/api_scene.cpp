// api_scene.cpp — the entry points of the C-ABI (include/doomgpu.h) that need no GPU: the error string and the version, the scene
// (dg_scene_*), one frame's lists and map lines on the host, the recorded walks, the box downscale on the host (dg_reduced_size,
// dg_reduce_host), the reduced depth and label planes (dg_plane_reduced_size, dg_reduce_planes_host), the observation tensors
// (dg_observed_size, dg_observe_host), the screen pictures (dg_scene_use_picture, dg_overlay_host), the depth planes, the label planes and boxes and a bundle's parts of caller-built lists on the host (dg_depth_lists_host, dg_label_lists_host,
// dg_bundle_lists_host: one rule, plane_lists_host), a bundle's slab layout (dg_bundle_layout), and the explored-map frames' host rules
// (dg_seen_words, dg_seen_lines_host, dg_seen_accumulate_host, dg_explored_map_host) and the player-centred map frames' (dg_ego_map_lines,
// dg_ego_map_host), and the line-of-sight queries' host twin (dg_sight_host, dg_sight_mobjs_host).  Everything that takes a dg_ctx: context.cpp (a slot's submissions), api_readback.cpp (what reads a slot) and
// api_device.cpp (the calls on a stream of the ctx's own).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "binner.hpp"
#include "ego_host.hpp"
#include "floor_map_host.hpp"
#include "explored_cover.hpp"
#include "frontend.hpp"
#include "map_things_host.hpp"
#include "observe_core.h"
#include "plane_core.h"
#include "plane_reduce_core.h"
#include "reduce_core.h"
#include "sight_host.hpp"
#include "slab_layout.h"
#include "walk.hpp"

using namespace dg;

thread_local std::string t_err;

// dg_build_lists and dg_build_lists_owners share the arena: one walk fills the lists and the owner tags alike.
static FrameArena &lists_arena() {
    static thread_local FrameArena arena;
    return arena;
}

// The spans of a column laid on in draw order, each row of a span that writes overwriting what is there (the plane walk of
// plane_kernels.hip reads the same order backwards): plane_core.h per pixel, with the parts the outputs ask for.
template <bool DEPTH, bool LABELS>
static void plane_frame_host(const BinnedFrame &bf, const uint32_t *tags, const DevScene &ds, const DevConsts &dk, size_t W, int16_t *dist, uint8_t *kd,
                             uint16_t *idp, uint8_t *clp) {
    for (size_t x = 0; x < W; x++)
        for (uint32_t j = bf.col_off[x]; j < bf.col_off[x + 1]; j++) {
            const DevSpan &sp = bf.spans[j];
            const PlaneSpan<DEPTH, LABELS> r = plane_resolve_span<DEPTH, LABELS>(sp, bf.hdr, bf.walls.data(), bf.planes.data(), tags, ds, dk);
            for (int32_t y = sp.ctop; y <= sp.cbot; y++) {
                int32_t d;
                uint32_t k, label;
                if (!plane_span_writes<DEPTH>(r, ds, dk, y, d, k, label)) continue;
                const size_t px = (size_t)y * W + x;
                if (dist) dist[px] = (int16_t)d;
                if (kd) kd[px] = (uint8_t)k;
                if (LABELS) { idp[px] = (uint16_t)label_index(label); clp[px] = (uint8_t)label_class(label); }
            }
        }
}

// dg_depth_lists_host, dg_label_lists_host and dg_bundle_lists_host: the binner (the same column-major, draw-ordered spans the GPU
// walks) and plane_frame_host for any subset of the five outputs, then the boxes by a plain scan of the label planes.  `labels`: the
// caller's lists come with owner tags, which are then checked (and the scene with them) whether or not a label output is there.  Every
// frame is checked before anything is written.
static int plane_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, const uint32_t *const *owners, int n, bool labels,
                            int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    const bool depth = distance || kind;
    if (!s || !frames) return set_err(DG_ERR_INVALID, "null argument");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384]");
    if (n < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    const Scene &sc = *s->sc;
    std::string err;
    int rc = labels ? check_label_scene(sc, err) : DG_OK;
    if (rc) return set_err(rc, err);
    const FrameConsts fk = make_consts(width, height);
    const DevConsts dk{fk.ARC, fk.GCFX, fk.CFX, fk.CFY, width, height};
    const BitmapInfo &sky = sc.bitmaps[(size_t)sc.sky_bitmap];
    const DevScene ds{nullptr, nullptr, sc.texel_idx.data(), sc.texel_opq.data(), nullptr, sky.texel_off, sky.w, sky.h, sky.has_holes};
    const size_t W = (size_t)width, H = (size_t)height, px = W * H, n_mobjs = sc.mobjs.size();
    std::vector<BinnedFrame> binned((size_t)n);
    std::vector<std::vector<uint32_t>> tags((size_t)n);
    for (int f = 0; f < n; f++) {
        dg_frame_lists fl = frames[f];
        fill_view_trig(fl.view);
        rc = bin_frame(sc, fk, fl, binned[(size_t)f], err);
        if (!rc && labels) rc = wall_owners(sc, fl, owners[f], tags[(size_t)f], err);
        if (rc) return set_err(rc, "frame " + std::to_string(f) + ": " + err);
    }
    std::vector<uint16_t> idp(labels ? px : 0);
    std::vector<uint8_t> clp(labels ? px : 0);
    std::vector<LabelRawBox> raw(n_mobjs);
    for (int f = 0; f < n; f++) {
        BinnedFrame &bf = binned[(size_t)f];
        bf.hdr.span_base = 0; bf.hdr.wall_base = 0; bf.hdr.plane_base = 0;
        int16_t *const dist = distance ? distance + (size_t)f * px : nullptr;
        uint8_t *const kd = kind ? kind + (size_t)f * px : nullptr;
        for (size_t i = 0; i < px; i++) {
            if (dist) dist[i] = (int16_t)DEPTH_FAR;
            if (kd) kd[i] = (uint8_t)KIND_NONE;
        }
        std::fill(idp.begin(), idp.end(), (uint16_t)0);
        std::fill(clp.begin(), clp.end(), (uint8_t)LABEL_NONE);
        const uint32_t *const t = tags[(size_t)f].data();
        if (depth && labels) plane_frame_host<true, true>(bf, t, ds, dk, W, dist, kd, idp.data(), clp.data());
        else if (depth) plane_frame_host<true, false>(bf, t, ds, dk, W, dist, kd, nullptr, nullptr);
        else if (labels) plane_frame_host<false, true>(bf, t, ds, dk, W, nullptr, nullptr, idp.data(), clp.data());
        if (id) std::memcpy(id + (size_t)f * px, idp.data(), px * sizeof(uint16_t));
        if (cls) std::memcpy(cls + (size_t)f * px, clp.data(), px);
        if (!boxes) continue;
        std::memset(raw.data(), 0, n_mobjs * sizeof(LabelRawBox));
        for (size_t y = 0; y < H; y++)
            for (size_t x = 0; x < W; x++) {
                if (clp[y * W + x] != (uint8_t)LABEL_MOBJ) continue;
                uint32_t *const b = raw[idp[y * W + x]].w;
                b[0]++;
                b[1] = std::max(b[1], (uint32_t)x + 1); b[2] = std::max(b[2], (uint32_t)y + 1);
                b[3] = std::max(b[3], (uint32_t)(W - x)); b[4] = std::max(b[4], (uint32_t)(H - y));
            }
        for (size_t m = 0; m < n_mobjs; m++) {
            int32_t x0, y0, x1, y1;
            dg_label_box &o = boxes[(size_t)f * n_mobjs + m];
            label_box_finish(raw[m], width, height, o.pixels, x0, y0, x1, y1);
            o.x0 = (int16_t)x0; o.y0 = (int16_t)y0; o.x1 = (int16_t)x1; o.y1 = (int16_t)y1;
        }
    }
    return DG_OK;
}

extern "C" {

const char *dg_last_error(void) { return t_err.c_str(); }
const char *dg_version(void) { return "doomgpu 0.6 (gfx950; ABI 4)"; }

int dg_scene_load_wad(const uint8_t *wad, size_t len, const char *map_name, dg_scene **out) {
    if (!wad || !map_name || !out) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    Scene *sc = load_scene_from_wad(wad, len, map_name, err);
    if (!sc) return set_err(DG_ERR_WAD, err);
    *out = new dg_scene{sc};
    return DG_OK;
}
void dg_scene_free(dg_scene *s) { if (s) { delete s->sc; delete s; } }
int dg_scene_player_start(const dg_scene *s, float *x, float *y, float *angle) {
    if (!s || !x || !y || !angle) return set_err(DG_ERR_INVALID, "null argument");
    if (!s->sc->has_start) return set_err(DG_ERR_WAD, "Could not find thing of type 1 (src/map/things.rs:46-55)");
    *x = s->sc->start_x; *y = s->sc->start_y; *angle = s->sc->start_angle;
    return DG_OK;
}
int dg_scene_floor_height_at(const dg_scene *s, float x, float y, float *h) {
    if (!s || !h) return set_err(DG_ERR_INVALID, "null argument");
    int sec = s->sc->sector_from_vertex(x, y);
    if (sec < 0) return 1;
    *h = (float)s->sc->sectors[(size_t)sec].floor_h;
    return DG_OK;
}
int dg_scene_sector_count(const dg_scene *s) { return s ? (int)s->sc->sectors.size() : DG_ERR_INVALID; }
int dg_scene_set_sector_light(dg_scene *s, int sector, int16_t light) {
    if (!s || sector < 0 || (size_t)sector >= s->sc->sectors.size()) return set_err(DG_ERR_INVALID, "bad sector");
    s->sc->sectors[(size_t)sector].light = light;
    s->sc->revision++;
    return DG_OK;
}
int dg_scene_mobj_count(const dg_scene *s) { return s ? (int)s->sc->mobjs.size() : DG_ERR_INVALID; }
int dg_scene_set_mobj_state(dg_scene *s, int mobj, const char *sprite, uint8_t frame, int full_bright) {
    if (!s || mobj < 0 || (size_t)mobj >= s->sc->mobjs.size()) return set_err(DG_ERR_INVALID, "bad map object");
    MapObjectRec &m = s->sc->mobjs[(size_t)mobj];
    s->sc->revision++;
    if (!sprite) { m.sprite_frame = -1; return DG_OK; }
    std::string err;
    int sf = s->sc->find_or_add_sprite_frame(sprite, frame, err);
    if (sf < 0) return set_err(DG_ERR_WAD, err);
    m.sprite_frame = sf; m.full_bright = full_bright;
    return DG_OK;
}
int dg_scene_texture_id(const dg_scene *s, const char *name) { return (s && name) ? s->sc->texture_id(name) : DG_ERR_INVALID; }
int dg_scene_flat_id(const dg_scene *s, const char *name, float ts) { return (s && name) ? s->sc->flat_id(name, ts) : DG_ERR_INVALID; }
int dg_scene_set_wall_effects(dg_scene *s, uint32_t flags) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    std::string err;
    const int rc = s->sc->set_wall_effects(flags, err);
    return rc ? set_err(rc, err) : DG_OK;
}
int dg_scene_wall_texture_id(const dg_scene *s, const char *name, float ts) { return (s && name) ? s->sc->wall_texture_id(name, ts) : DG_ERR_INVALID; }
int dg_scene_set_light_effects(dg_scene *s, uint32_t flags, uint64_t seed) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    std::string err;
    const int rc = s->sc->set_light_effects(flags, seed, err);
    return rc ? set_err(rc, err) : DG_OK;
}
int dg_scene_sector_lights_at(const dg_scene *s, float ts, int16_t *out, int n) {
    if (!s || !out) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.sectors.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_sector_count");
    for (size_t i = 0; i < sc.sectors.size(); i++) out[i] = sc.sectors[i].light;
    const LightFx &fx = sc.fx.light;
    if (fx.on())
        for (size_t r = 0; r < fx.recs.size(); r++) out[fx.recs[r].sector] = fx.level(r, ts);
    return DG_OK;
}
int dg_scene_set_mobj_thinkers(dg_scene *s, uint32_t flags, const dg_state_rec *states, int n_states, const dg_mobj_info_rec *infos, int n_infos) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    std::string err;
    const int rc = s->sc->set_mobj_thinkers(flags, states, n_states, infos, n_infos, err);
    return rc ? set_err(rc, err) : DG_OK;
}
int dg_scene_mobj_event(dg_scene *s, int what, float ts) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    std::string err;
    const int rc = s->sc->mobj_event(what, ts, err);
    return rc ? set_err(rc, err) : DG_OK;
}
int dg_scene_mobj_states_at(const dg_scene *s, float ts, dg_mobj_state *out, int n) {
    if (!s || !out) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.mobjs.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_mobj_count");
    for (size_t i = 0; i < sc.mobjs.size(); i++)
        out[i] = dg_mobj_state{(int32_t)i, sc.mobjs[i].sprite_frame < 0 ? -1 : sc.mobjs[i].sprite_frame, sc.mobjs[i].sprite_frame < 0 ? 0 : (sc.mobjs[i].full_bright ? 1 : 0), 0};
    const MobjFx &fx = sc.fx.mobj;
    if (fx.fits(sc))
        for (uint32_t i : fx.driven) mfx_decode(fx.value(i, ts), out[i].sprite_frame, out[i].full_bright);
    return DG_OK;
}
int dg_scene_sprite_bitmap_id(const dg_scene *s, const char *sprite, uint8_t frame, uint8_t rot) {
    return (s && sprite) ? s->sc->sprite_bitmap_id(sprite, frame, rot) : DG_ERR_INVALID;
}
int dg_scene_bitmap_size(const dg_scene *s, int bitmap, int *w, int *h) {
    if (!s || bitmap < 0 || (size_t)bitmap >= s->sc->bitmaps.size()) return set_err(DG_ERR_INVALID, "bad bitmap id");
    if (w) *w = s->sc->bitmaps[(size_t)bitmap].w;
    if (h) *h = s->sc->bitmaps[(size_t)bitmap].h;
    return DG_OK;
}

int dg_build_lists(const dg_scene *s, int width, int height, const dg_view *view, dg_frame_lists *out) {
    if (!s || !view || !out) return set_err(DG_ERR_INVALID, "null argument");
    dg_view v = *view;
    fill_view_trig(v);
    std::string err;
    int rc = build_frame_lists(*s->sc, width, height, v, lists_arena(), *out, err, {}, &s->sc->fx);
    return rc ? set_err(rc, err) : DG_OK;
}

int dg_build_lists_owners(const dg_scene *s, int width, int height, const dg_view *view, dg_frame_lists *out, const uint32_t **owners) {
    if (!s || !view || !out || !owners) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    int rc = check_label_scene(*s->sc, err);
    if (rc) return set_err(rc, err);
    rc = dg_build_lists(s, width, height, view, out);
    if (rc) return rc;
    *owners = lists_arena().owners.data();
    return DG_OK;
}

int dg_build_lists_poses(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, dg_frame_lists *out, const uint32_t **owners) {
    return dg_build_lists_sectors(s, width, height, view, poses, nullptr, out, owners);
}

int dg_scene_sector_heights(const dg_scene *s, int16_t *floor, int16_t *ceiling, int n) {
    if (!s || !floor || !ceiling) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.sectors.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_sector_count");
    for (size_t i = 0; i < sc.sectors.size(); i++) { floor[i] = sc.sectors[i].floor_h; ceiling[i] = sc.sectors[i].ceil_h; }
    return DG_OK;
}

int dg_build_lists_sectors(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, const dg_view_sectors *sectors, dg_frame_lists *out,
                           const uint32_t **owners) {
    return dg_build_lists_surfaces(s, width, height, view, poses, sectors, nullptr, out, owners);
}

int dg_scene_use_texture(dg_scene *s, const char *name) {
    if (!s || !name) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int id = s->sc->use_texture(name, err);
    return id == TEX_UNKNOWN ? set_err(DG_ERR_WAD, err) : id;
}

int dg_scene_use_flat(dg_scene *s, const char *name) {
    if (!s || !name) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int h = s->sc->use_flat(name, err);
    return h < 0 ? set_err(DG_ERR_WAD, err) : h;
}

int dg_scene_use_picture(dg_scene *s, const char *name) {
    if (!s || !name) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int h = s->sc->use_picture(name, err);
    return h < 0 ? set_err(DG_ERR_WAD, err) : h;
}

int dg_scene_picture_count(const dg_scene *s) { return s ? (int)s->sc->pictures.size() : set_err(DG_ERR_INVALID, "null scene"); }

int dg_scene_picture_info(const dg_scene *s, int picture, int32_t *w, int32_t *h, int32_t *left, int32_t *top) {
    if (!s || picture < 0 || (size_t)picture >= s->sc->pictures.size()) return set_err(DG_ERR_INVALID, "not a picture handle of the scene");
    const BitmapInfo &b = s->sc->bitmaps[(size_t)s->sc->pictures[(size_t)picture]];
    if (w) *w = b.w;
    if (h) *h = b.h;
    if (left) *left = b.left_offset;
    if (top) *top = b.top_offset;
    return DG_OK;
}

// The walk of dg_overlay_tiles (overlay_kernels.hip) on the host: the plan's rectangle records tile by tile, and per pixel the items from
// the last to the first until one has a Some texel there.
int dg_overlay_host(const dg_scene *s, uint8_t *frames, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first) {
    if (!s || !frames) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    OvlPlan plan;
    if (const int rc = overlay_checked_plan(overlay_pictures(sc), width, height, n_frames, items, first, plan)) return rc;
    const size_t W = (size_t)width, frame_bytes = 3u * W * (size_t)height;
    for (const OvlRect &r : plan.rects)
        for (uint32_t t = r.tile0; t < r.tile0 + r.tiles; t++) {
            const int32_t tx0 = (int32_t)(r.x0 + (t % r.tiles_x) * OVL_TILE_W), ty0 = (int32_t)(r.y0 + (t / r.tiles_x) * OVL_TILE_H);
            for (int32_t py = ty0; py < ty0 + (int32_t)OVL_TILE_H && py < (int32_t)r.y1; py++)
                for (int32_t px = tx0; px < tx0 + (int32_t)OVL_TILE_W && px < (int32_t)r.x1; px++)
                    for (uint32_t k = r.item1; k > r.item0; k--) {
                        const OvlItem &it = plan.items[k - 1u];
                        if (!ovl_covers(it, px, py)) continue;
                        const uint32_t o = ovl_texel(it, px, py);
                        if (!sc.texel_opq[o]) continue;
                        const uint8_t *const pal = sc.palette + 3u * sc.texel_idx[o];
                        const uint32_t rgb = ovl_colour(it, (uint32_t)pal[0] | ((uint32_t)pal[1] << 8) | ((uint32_t)pal[2] << 16));
                        uint8_t *const p = frames + (size_t)r.frame * frame_bytes + ((size_t)py * W + (size_t)px) * 3u;
                        p[0] = (uint8_t)rgb; p[1] = (uint8_t)(rgb >> 8); p[2] = (uint8_t)(rgb >> 16);
                        break;
                    }
        }
    return DG_OK;
}

int dg_scene_sidedef_count(const dg_scene *s) { return s ? (int)s->sc->sidedefs.size() : set_err(DG_ERR_INVALID, "null scene"); }

int dg_scene_sidedef_surfaces(const dg_scene *s, dg_side_surface *out, int n) {
    if (!s || !out) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.sidedefs.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_sidedef_count");
    for (size_t i = 0; i < sc.sidedefs.size(); i++) {
        const SidedefRec &r = sc.sidedefs[i];
        out[i] = dg_side_surface{(int32_t)i, r.middle, r.lower, r.upper, (int32_t)r.xoff, (int32_t)r.yoff};
    }
    return DG_OK;
}

int dg_scene_sector_flats(const dg_scene *s, dg_sector_flats *out, int n) {
    if (!s || !out) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.sectors.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_sector_count");
    for (size_t i = 0; i < sc.sectors.size(); i++) out[i] = dg_sector_flats{(int32_t)i, sc.fs_flats[i].floor, sc.fs_flats[i].ceil};
    return DG_OK;
}

int dg_build_lists_surfaces(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, const dg_view_sectors *sectors,
                            const dg_view_surfaces *surfaces, dg_frame_lists *out, const uint32_t **owners) {
    if (!s || !view || !out) return set_err(DG_ERR_INVALID, "null argument");
    const ViewInputs in{nullptr, poses, sectors, surfaces};
    std::string err;
    if (!check_view_inputs(in, err)) return set_err(DG_ERR_INVALID, err);
    int rc = owners ? check_label_scene(*s->sc, err) : DG_OK;
    if (rc) return set_err(rc, err);
    dg_view v = *view;
    fill_view_trig(v);
    rc = build_frame_lists(*s->sc, width, height, v, lists_arena(), *out, err, in, &s->sc->fx);
    if (rc) return set_err(rc, err);
    if (owners) *owners = lists_arena().owners.data();
    return DG_OK;
}

int dg_scene_sectors_at(const dg_scene *s, const float *x, const float *y, int n, int32_t *sector_out) {
    if (!s || n < 0 || (n > 0 && (!x || !y || !sector_out))) return set_err(DG_ERR_INVALID, n < 0 ? "n must not be negative" : "null argument");
    for (int i = 0; i < n; i++) sector_out[i] = s->sc->sector_from_vertex(x[i], y[i]);
    return DG_OK;
}

int dg_scene_mobj_poses(const dg_scene *s, dg_mobj_placed *out, int n) {
    if (!s || !out) return set_err(DG_ERR_INVALID, "null argument");
    const Scene &sc = *s->sc;
    if (n < 0 || (size_t)n != sc.mobjs.size()) return set_err(DG_ERR_INVALID, "n must equal dg_scene_mobj_count");
    for (size_t i = 0; i < sc.mobjs.size(); i++) out[i] = dg_mobj_placed{sc.mobjs[i].x, sc.mobjs[i].y, sc.mobjs[i].angle, sc.mobjs[i].sector};
    return DG_OK;
}

int dg_scene_sprite_frame(dg_scene *s, const char *sprite, uint8_t frame) {
    if (!s || !sprite) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int sf = s->sc->find_or_add_sprite_frame(sprite, frame, err);
    return sf < 0 ? set_err(DG_ERR_WAD, err) : sf;
}

int dg_map_lines(const dg_scene *s, int width, int height, const dg_view *view, dg_map_line *out, int cap) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    dg_view v{};
    if (view) { v = *view; fill_view_trig(v); }
    static thread_local std::vector<dg_map_line> lines;
    std::string err;
    const int rc = map_frame_lines(*s->sc, width, height, view ? &v : nullptr, lines, err);
    if (rc) return set_err(rc, err);
    if (out && cap >= 0 && (size_t)cap >= lines.size() && !lines.empty()) std::memcpy(out, lines.data(), lines.size() * sizeof(dg_map_line));
    return (int)lines.size();
}

int dg_walk_create(const dg_scene *s, const dg_walk_desc *d, dg_walk **out) {
    if (!s || !d || !out) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int rc = walk_create(*s->sc, *d, out, err);
    return rc ? set_err(rc, err) : DG_OK;
}
void dg_walk_free(dg_walk *w) { delete w; }
int dg_walk_tics(const dg_walk *w) { return w ? (int)w->tics() : set_err(DG_ERR_INVALID, "null argument"); }
int dg_walk_probe_count(const dg_walk *w) { return w ? (int)w->px.size() : set_err(DG_ERR_INVALID, "null argument"); }
int dg_walk_floors(dg_walk *w, float *out, int n) {
    if (!w || !out) return set_err(DG_ERR_INVALID, "null argument");
    if (n < 0 || (size_t)n != w->pose.size()) return set_err(DG_ERR_INVALID, "n must be tics + 1");
    w->locate_host();
    std::memcpy(out, w->floors.data(), (size_t)n * sizeof(float));
    return DG_OK;
}
int dg_walk_views(dg_walk *w, const float *timestamps, int n, dg_view *out) {
    if (!w || n < 0 || (n > 0 && (!timestamps || !out))) return set_err(DG_ERR_INVALID, "null argument");
    w->locate_host();
    for (int i = 0; i < n; i++) w->view_at(timestamps[i], out[i]);
    return DG_OK;
}

int dg_reduced_size(int width, int height, const dg_reduce_desc *desc, int *out_w, int *out_h, size_t *bytes_per_frame) {
    if (!desc) return set_err(DG_ERR_INVALID, "null argument");
    if (width < 1 || height < 1) return set_err(DG_ERR_INVALID, "width and height must be positive");
    if (!reduce_desc_ok(*desc)) return set_err(DG_ERR_INVALID, "reduce descriptor: fx and fy in 1..16, a known format, reserved 0");
    if (out_w) *out_w = (int)reduce_out_dim((uint32_t)width, desc->fx);
    if (out_h) *out_h = (int)reduce_out_dim((uint32_t)height, desc->fy);
    if (bytes_per_frame) *bytes_per_frame = reduce_frame_bytes((uint32_t)width, (uint32_t)height, *desc);
    return DG_OK;
}

int dg_reduce_host(const uint8_t *src_rgb24, int width, int height, int n_frames, const dg_reduce_desc *desc, uint8_t *dst) {
    if (!src_rgb24 || !dst) return set_err(DG_ERR_INVALID, "null argument");
    if (n_frames < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    const int rc = dg_reduced_size(width, height, desc, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const uint32_t W = (uint32_t)width, H = (uint32_t)height, fx = desc->fx, fy = desc->fy;
    const uint32_t oW = reduce_out_dim(W, fx), oH = reduce_out_dim(H, fy);
    const bool gray = desc->format == DG_REDUCE_GRAY8;
    const size_t row = (size_t)3 * W;
    for (int f = 0; f < n_frames; f++) {
        const uint8_t *const frame = src_rgb24 + (size_t)f * row * H;
        for (uint32_t oy = 0; oy < oH; oy++) {
            uint32_t y0;
            const uint32_t ny = reduce_box(oy, fy, H, y0);
            for (uint32_t ox = 0; ox < oW; ox++) {
                uint32_t x0;
                const uint32_t nx = reduce_box(ox, fx, W, x0), n = nx * ny, rcp = reduce_rcp(n);
                uint32_t px[3];
                for (uint32_t c = 0; c < 3; c++) {
                    uint32_t s = 0;
                    for (uint32_t y = y0; y < y0 + ny; y++)
                        for (uint32_t x = x0; x < x0 + nx; x++) s += frame[(size_t)y * row + (size_t)3 * x + c];
                    px[c] = reduce_round(s, n, rcp);
                }
                if (gray) *dst++ = (uint8_t)reduce_luma(px[0], px[1], px[2]);
                else { *dst++ = (uint8_t)px[0]; *dst++ = (uint8_t)px[1]; *dst++ = (uint8_t)px[2]; }
            }
        }
    }
    return DG_OK;
}

int dg_plane_reduced_size(int width, int height, const dg_plane_reduce_desc *desc, int *out_w, int *out_h) {
    const int rc = check_plane_reduce(width, height, 0, desc);
    if (rc) return rc;
    if (out_w) *out_w = (int)reduce_out_dim((uint32_t)width, desc->fx);
    if (out_h) *out_h = (int)reduce_out_dim((uint32_t)height, desc->fy);
    return DG_OK;
}

int dg_reduce_planes_host(int width, int height, int n_frames, const dg_plane_reduce_desc *desc,
                          const int16_t *distance, const uint8_t *kind, const uint16_t *id, const uint8_t *cls,
                          int16_t *o_distance, uint8_t *o_kind, uint16_t *o_id, uint8_t *o_cls) {
    int rc = check_plane_reduce(width, height, n_frames, desc);
    if (!rc) rc = check_plane_pairs(*desc, distance, kind, id, cls, o_distance, o_kind, o_id, o_cls);
    if (rc) return rc;
    const uint32_t W = (uint32_t)width, H = (uint32_t)height, fx = desc->fx, fy = desc->fy;
    const uint32_t oW = reduce_out_dim(W, fx), oH = reduce_out_dim(H, fy);
    const size_t px = (size_t)W * H;
    size_t o = 0;
    for (int f = 0; f < n_frames; f++) {
        const size_t base = (size_t)f * px;
        for (uint32_t oy = 0; oy < oH; oy++) {
            uint32_t y0;
            const uint32_t ny = reduce_box(oy, fy, H, y0);
            for (uint32_t ox = 0; ox < oW; ox++, o++) {
                uint32_t x0, x, y;
                const uint32_t nx = reduce_box(ox, fx, W, x0);
                if (desc->rule == DG_PLANE_NEAREST) {
                    const uint32_t key = plane_nearest_key(distance + base, W, x0, nx, y0, ny);
                    x = x0 + plane_key_rx(key); y = y0 + plane_key_ry(key);
                } else {
                    x = plane_point(ox, fx, W); y = plane_point(oy, fy, H);
                }
                const size_t s = base + (size_t)y * W + x;
                if (o_distance) o_distance[o] = distance[s];
                if (o_kind) o_kind[o] = kind[s];
                if (o_id) o_id[o] = id[s];
                if (o_cls) o_cls[o] = cls[s];
            }
        }
    }
    return DG_OK;
}

int dg_observed_size(int width, int height, const dg_obs_desc *desc, int *channels, int *out_h, int *out_w, int *element_bytes) {
    const int rc = check_observe(width, height, desc);
    if (rc) return rc;
    if (channels) *channels = (int)obs_channels(desc->source);
    if (out_h) *out_h = (int)reduce_out_dim((uint32_t)height, desc->fy);
    if (out_w) *out_w = (int)reduce_out_dim((uint32_t)width, desc->fx);
    if (element_bytes) *element_bytes = (int)obs_element_bytes(desc->dtype);
    return DG_OK;
}

// The integer values are dg_reduce_host's / dg_reduce_planes_host's own, frame by frame; what is added is observe_core.h's.
int dg_observe_host(const void *src, int width, int height, int n_frames, const dg_obs_desc *desc, void *dst, const int64_t strides[4]) {
    int rc = check_observe_call(src, width, height, n_frames, desc, dst, strides);
    if (rc) return rc;
    const uint32_t C = obs_channels(desc->source), oW = reduce_out_dim((uint32_t)width, desc->fx), oH = reduce_out_dim((uint32_t)height, desc->fy);
    const size_t px = (size_t)width * (size_t)height, opx = (size_t)oW * oH;
    std::vector<uint8_t> bytes;
    std::vector<int16_t> dist;
    const dg_reduce_desc rd{desc->fx, desc->fy, desc->source == DG_OBS_GRAY ? (uint32_t)DG_REDUCE_GRAY8 : (uint32_t)DG_REDUCE_RGB24, 0u};
    const dg_plane_reduce_desc pd{desc->fx, desc->fy, desc->rule, 0u};
    if (desc->source == DG_OBS_DISTANCE) dist.resize(opx);
    else bytes.resize(opx * C);
    for (int f = 0; f < n_frames; f++) {
        if (desc->source == DG_OBS_DISTANCE)
            rc = dg_reduce_planes_host(width, height, 1, &pd, static_cast<const int16_t *>(src) + (size_t)f * px, nullptr, nullptr, nullptr, dist.data(), nullptr, nullptr, nullptr);
        else
            rc = dg_reduce_host(static_cast<const uint8_t *>(src) + (size_t)f * px * 3u, width, height, 1, &rd, bytes.data());
        if (rc) return rc;
        for (uint32_t oy = 0; oy < oH; oy++)
            for (uint32_t ox = 0; ox < oW; ox++)
                for (uint32_t c = 0; c < C; c++) {
                    const size_t i = (size_t)oy * oW + ox;
                    const int32_t v = desc->source == DG_OBS_DISTANCE ? (int32_t)dist[i] : (int32_t)bytes[i * C + c];
                    obs_put(*desc, dst, (int64_t)f * strides[0] + (int64_t)c * strides[1] + (int64_t)oy * strides[2] + (int64_t)ox * strides[3], v);
                }
    }
    return DG_OK;
}

int dg_depth_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, int n, int16_t *distance, uint8_t *kind) {
    return plane_lists_host(s, width, height, frames, nullptr, n, false, distance, kind, nullptr, nullptr, nullptr);
}

int dg_label_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, const uint32_t *const *owners, int n,
                        uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    if (!s || !frames || !owners) return set_err(DG_ERR_INVALID, "null argument");
    return plane_lists_host(s, width, height, frames, owners, n, true, nullptr, nullptr, id, cls, boxes);
}

int dg_bundle_layout(int width, int height, int n, uint32_t what, dg_bundle_offsets *out) {
    if (!out) return set_err(DG_ERR_INVALID, "null argument");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384]");
    if (n <= 0) return set_err(DG_ERR_INVALID, "bad frame count");
    if (what == 0 || (what & ~BUNDLE_ALL)) return set_err(DG_ERR_INVALID, "what must be a non-empty set of DG_BUNDLE_COLOUR, DG_BUNDLE_DEPTH, DG_BUNDLE_LABELS");
    const BundleLayout L = bundle_layout((size_t)n, (size_t)width, (size_t)height, what);
    *out = dg_bundle_offsets{L.colour, L.distance, L.kind, L.id, L.cls, L.total};
    return DG_OK;
}

int dg_bundle_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, const uint32_t *const *owners, int n,
                         int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes) {
    const bool labels = id || cls || boxes;
    if (!s || !frames) return set_err(DG_ERR_INVALID, "null argument");
    if (labels && !owners) return set_err(DG_ERR_INVALID, "null owners: the label outputs need the owner tags");
    return plane_lists_host(s, width, height, frames, owners, n, labels, distance, kind, id, cls, boxes);
}

int dg_seen_words(const dg_scene *s) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    return (int)seen_words((uint32_t)s->sc->linedefs.size());
}

int dg_seen_lines_host(const dg_scene *s, int width, int height, int n, const uint16_t *id, const uint8_t *cls, uint32_t *seen) {
    const int rc = check_seen_lines(s ? s->sc : nullptr, width, height, n, id, cls, seen);
    if (rc) return rc;
    const Scene &sc = *s->sc;
    const size_t px = (size_t)width * (size_t)height, words = seen_words((uint32_t)sc.linedefs.size());
    const uint32_t n_segs = (uint32_t)sc.segs.size();
    std::memset(seen, 0, (size_t)n * words * sizeof(uint32_t));
    for (int f = 0; f < n; f++) {
        uint32_t *const row = seen + (size_t)f * words;
        for (size_t p = (size_t)f * px; p < (size_t)(f + 1) * px; p++) {
            if (!seen_pixel(cls[p], id[p], n_segs)) continue;
            const uint32_t line = (uint32_t)sc.segs[id[p]].linedef;
            row[line >> 5] |= 1u << (line & 31u);
        }
    }
    return DG_OK;
}

int dg_seen_accumulate_host(int words, int n, int run_len, const uint32_t *carry_in, const uint32_t *seen, uint32_t *upto, uint32_t *total,
                            uint32_t *fresh, uint32_t *carry_out) {
    const int rc = check_seen_runs(words, n, run_len);
    if (rc) return rc;
    if (n > 0 && !seen) return set_err(DG_ERR_INVALID, "null seen rows");
    const size_t Wd = (size_t)words;
    std::vector<uint32_t> acc(Wd);
    for (int run = 0; run < n / run_len; run++) {
        for (size_t w = 0; w < Wd; w++) acc[w] = carry_in ? carry_in[(size_t)run * Wd + w] : 0u;
        for (int f = run * run_len; f < (run + 1) * run_len; f++) {
            uint32_t t = 0, fr = 0;
            for (size_t w = 0; w < Wd; w++) {
                const uint32_t next = acc[w] | seen[(size_t)f * Wd + w];
                fr += popcount32(next & ~acc[w]);
                t += popcount32(next);
                acc[w] = next;
                if (upto) upto[(size_t)f * Wd + w] = next;
            }
            if (total) total[f] = t;
            if (fresh) fresh[f] = fr;
        }
        if (carry_out) std::memcpy(carry_out + (size_t)run * Wd, acc.data(), Wd * sizeof(uint32_t));
    }
    return DG_OK;
}

// The literal rule: black, the drawn linedefs whose bit is set in LINEDEFS order, then the arrow, every point through map_seg_point.
int dg_explored_map_host(const dg_scene *s, int width, int height, const dg_view *view, const uint32_t *mask_row, uint8_t *rgb24_out) {
    if (!s || !mask_row || !rgb24_out) return set_err(DG_ERR_INVALID, "null argument");
    dg_view v{};
    if (view) { v = *view; fill_view_trig(v); }
    std::vector<dg_map_line> lines;
    std::string err;
    const int rc = map_frame_lines(*s->sc, width, height, view ? &v : nullptr, lines, err);
    if (rc) return set_err(rc, err);
    const std::vector<uint32_t> ids = explored_line_ids(*s->sc);
    map_draw_lines_host(lines.data(), lines.size(), width, height, rgb24_out,
                        [&](size_t k) { return k >= ids.size() || ((mask_row[ids[k] >> 5] >> (ids[k] & 31u)) & 1u); });       // (k >= ids.size(): the arrow)
    return DG_OK;
}

// What dg_ego_map_lines and dg_ego_map_host do alike: the contract's checks, then the frame's lines (ego_host.hpp).
static int ego_lines_checked(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                             std::vector<dg_map_line> &lines) {
    if (!s || !view || !params) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    int rc = ego_check_call(*s->sc, width, height, params, err);
    if (rc) return set_err(rc, err);
    dg_view v = *view;
    fill_view_trig(v);
    rc = ego_check_view(v, err);
    if (!rc) rc = ego_frame_lines(*s->sc, width, height, v, *params, mask_row, lines, err);
    return rc ? set_err(rc, err) : DG_OK;
}

int dg_ego_map_lines(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, dg_map_line *out, int cap) {
    static thread_local std::vector<dg_map_line> lines;
    const int rc = ego_lines_checked(s, width, height, view, params, nullptr, lines);
    if (rc) return rc;
    if (out && cap >= 0 && (size_t)cap >= lines.size() && !lines.empty()) std::memcpy(out, lines.data(), lines.size() * sizeof(dg_map_line));
    return (int)lines.size();
}

// The literal rule: black, the surviving lines in draw order, every point through map_seg_point.
int dg_ego_map_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                    uint8_t *rgb24_out) {
    if (!rgb24_out) return set_err(DG_ERR_INVALID, "null argument");
    std::vector<dg_map_line> lines;
    const int rc = ego_lines_checked(s, width, height, view, params, mask_row, lines);
    if (rc) return rc;
    map_draw_lines_host(lines.data(), lines.size(), width, height, rgb24_out, [](size_t) { return true; });
    return DG_OK;
}

// The literal rule of the floor-textured frames (floor_map_host.hpp), with the scene's effects as last set.  Everything is checked
// before the first byte of rgb24_out is written.
int dg_floor_map_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                      const dg_view_state *state, const dg_view_surfaces *surfaces, uint8_t *rgb24_out) {
    if (!s || !view || !params || !rgb24_out) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    int rc = floor_check_call(*s->sc, width, height, params, err);
    if (rc) return set_err(rc, err);
    dg_view v = *view;
    fill_view_trig(v);
    rc = ego_check_view(v, err);
    if (!rc) rc = floor_frame_host(*s->sc, &s->sc->fx.light, width, height, v, *params, mask_row, state, surfaces, rgb24_out, err);
    return rc ? set_err(rc, err) : DG_OK;
}

int dg_scene_set_map_markers(dg_scene *s, const dg_map_marker *markers, int n) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    std::string err;
    const int rc = thing_check_markers(markers, n, s->sc->mobjs.size(), err);
    if (rc) return set_err(rc, err);
    if (markers) s->sc->markers.assign(markers, markers + n);
    else s->sc->markers.clear();
    return DG_OK;
}

// What the three thing functions do alike: the contract's checks (floor: the floor-textured frames' too), then the view with its trig.
static int thing_call_checked(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, bool floor, dg_view &v) {
    if (!s || !view || !params) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    int rc = floor ? floor_check_call(*s->sc, width, height, params, err) : ego_check_call(*s->sc, width, height, params, err);
    if (!rc) rc = thing_check_call(*s->sc, err);
    if (rc) return set_err(rc, err);
    v = *view;
    fill_view_trig(v);
    rc = ego_check_view(v, err);
    return rc ? set_err(rc, err) : DG_OK;
}

int dg_map_thing_lines(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const dg_view_state *state,
                       const dg_view_poses *poses, dg_map_line *out, int cap) {
    dg_view v;
    int rc = thing_call_checked(s, width, height, view, params, false, v);
    if (rc) return rc;
    const Scene &sc = *s->sc;
    static thread_local std::vector<dg_map_line> lines;
    lines.clear();
    std::string err;
    rc = thing_view_lines(sc, thing_markers(sc, sc.markers), &sc.fx.mobj, width, height, v, *params, state, poses, lines, err);
    if (rc) return set_err(rc, err);
    if (out && cap >= 0 && (size_t)cap >= lines.size() && !lines.empty()) std::memcpy(out, lines.data(), lines.size() * sizeof(dg_map_line));
    return (int)lines.size();
}

// The literal rule: black, the linedefs, the markers and the arrow in draw order, every point through map_seg_point.
int dg_ego_map_things_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                           const dg_view_state *state, const dg_view_poses *poses, uint8_t *rgb24_out) {
    if (!rgb24_out) return set_err(DG_ERR_INVALID, "null argument");
    dg_view v;
    int rc = thing_call_checked(s, width, height, view, params, false, v);
    if (rc) return rc;
    const Scene &sc = *s->sc;
    std::vector<dg_map_line> lines;
    std::string err;
    rc = thing_all_lines(sc, thing_markers(sc, sc.markers), &sc.fx.mobj, width, height, v, *params, mask_row, state, poses, lines, err);
    if (rc) return set_err(rc, err);
    thing_draw_lines_host(lines, width, height, rgb24_out, nullptr);
    return DG_OK;
}

// ... and the floor under every pixel none of them wrote (a black marker's pixel is the marker's, not the floor's).
int dg_floor_map_things_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                             const dg_view_state *state, const dg_view_surfaces *surfaces, const dg_view_poses *poses, uint8_t *rgb24_out) {
    if (!rgb24_out) return set_err(DG_ERR_INVALID, "null argument");
    dg_view v;
    int rc = thing_call_checked(s, width, height, view, params, true, v);
    if (rc) return rc;
    const Scene &sc = *s->sc;
    std::vector<dg_map_line> lines;
    std::string err;
    rc = thing_all_lines(sc, thing_markers(sc, sc.markers), &sc.fx.mobj, width, height, v, *params, mask_row, state, poses, lines, err);
    FloorFrameHost F;
    if (!rc) rc = floor_frame_prepare(sc, &sc.fx.light, v, mask_row, state, surfaces, F, err);
    if (rc) return set_err(rc, err);
    std::vector<uint8_t> covered;
    thing_draw_lines_host(lines, width, height, rgb24_out, &covered);
    floor_frame_fill(sc, F, width, height, v, *params, mask_row, rgb24_out, [&](size_t at) { return covered[at] != 0; });
    return DG_OK;
}

int dg_scene_bsp_depth(const dg_scene *s) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    return (int)sight_scene_depth(*s->sc);
}

int dg_sight_words(const dg_scene *s) {
    if (!s) return set_err(DG_ERR_INVALID, "null scene");
    return (int)sight_words(*s->sc);
}

// The host twin of dg_sight_queries: sight_core.h's traversal, one query after the other, on a stack as deep as the scene is.
int dg_sight_host(const dg_scene *s, const dg_view_sectors *sectors, int n_frames, const dg_sight_query *q, int n, uint8_t *visible_out) {
    std::string err;
    int rc = sight_check_queries(s ? s->sc : nullptr, n_frames, q, n, visible_out, err);
    if (rc) return set_err(rc, err);
    if (n == 0) return DG_OK;
    const Scene &sc = *s->sc;
    LatestHeights latest;
    std::vector<SectorEntry> entries;
    if ((rc = sight_sector_entries(sc, sectors, n_frames, latest, entries, err))) return set_err(rc, err);
    SightHostTables H;
    sight_tables(sc, H);
    std::vector<FsHeights> rows;
    const uint32_t row_frames = sight_height_rows(sc, entries, n_frames, rows);
    const SightTables T = sight_tables_host(sc, H, rows.data(), row_frames);
    SightHostStack stack;
    for (int i = 0; i < n; i++) {
        stack.v.clear();
        visible_out[i] = sight_query(T, q[i], stack);
    }
    return DG_OK;
}

// The host twin of dg_sight_mobjs: every (view, map object) pair's query through the same traversal, its bit into the view's row.
int dg_sight_mobjs_host(const dg_scene *s, const dg_view *views, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, float eye_height,
                        const float *mobj_height, uint32_t *visible_out) {
    std::string err;
    int rc = sight_check_mobjs(s ? s->sc : nullptr, views, n, mobj_height, visible_out, err);
    if (rc) return set_err(rc, err);
    if (n == 0) return DG_OK;
    const Scene &sc = *s->sc;
    LatestHeights latest_h;
    LatestPoses latest_p;
    std::vector<SectorEntry> h_entries;
    std::vector<PoseEntry> p_entries;
    if ((rc = sight_sector_entries(sc, sectors, n, latest_h, h_entries, err))) return set_err(rc, err);
    if ((rc = sight_pose_entries(sc, poses, n, latest_p, p_entries, err))) return set_err(rc, err);
    const size_t M = sc.mobjs.size(), words = sight_words(sc);
    if (M == 0) return DG_OK;
    SightHostTables H;
    sight_tables(sc, H);
    std::vector<FsHeights> rows;
    std::vector<FsMobj> pose_rows;
    const uint32_t row_frames = sight_height_rows(sc, h_entries, n, rows), pose_frames = sight_pose_rows(sc, p_entries, n, pose_rows);
    const SightTables T = sight_tables_host(sc, H, rows.data(), row_frames);
    std::vector<SightView> sv;
    sight_views(views, n, eye_height, sv);
    SightHostStack stack;
    std::fill(visible_out, visible_out + (size_t)n * words, 0u);
    for (int f = 0; f < n; f++) {
        const FsMobj *const pr = pose_rows.data() + (pose_frames > 1 ? (size_t)f * M : (size_t)0);
        for (size_t m = 0; m < M; m++) {
            dg_sight_query q;
            if (!sight_mobj_query(T, f, sv[(size_t)f], pr[m], mobj_height[m], q)) continue;
            stack.v.clear();
            if (sight_query(T, q, stack)) visible_out[(size_t)f * words + (m >> 5)] |= 1u << (m & 31u);
        }
    }
    return DG_OK;
}

}  // extern "C"
