// api_scene.cpp — the entry points of the C-ABI (include/doomgpu.h) that need no GPU: the error string and the version, the scene
// (dg_scene_*), one frame's lists and map lines on the host, and the recorded walks.  Everything that takes a dg_ctx: context.cpp.
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "frontend.hpp"
#include "walk.hpp"

using namespace dg;

thread_local std::string t_err;

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
    static thread_local FrameArena arena;
    dg_view v = *view;
    fill_view_trig(v);
    std::string err;
    int rc = build_frame_lists(*s->sc, width, height, v, arena, *out, err, nullptr, &s->sc->fx);
    return rc ? set_err(rc, err) : DG_OK;
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

}  // extern "C"
