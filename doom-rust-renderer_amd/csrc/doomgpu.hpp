// doomgpu.hpp — host-side mirror of the reference's draw API for this path, in C++ because the reference is compiled
// code and no Rust toolchain exists in this image (the Rust binding is shipped as source under rust/).
//
//   reference (src/renderer/pixels.rs:5-47, src/renderer/mod.rs:27-58,118-136, src/game.rs:40-45,505-525)      here
//   Pixels::new() / .pixels / clear / set / draw_vertical_line                                          doom::Pixels
//   Player { position, floor_height, angle }                                                            doom::Player
//   Map + MapObjects + Textures + Sprites + sky_texture + Flats + Palette (borrowed by Renderer::new)   doom::World
//   Renderer::new(&mut pixels, .., &player, timestamp).render()                                         doom::Renderer
//   Game::render with viewing_map (draw_map_linedefs + draw_map_player, src/game.rs:229-309,491-499)   doom::Renderer::render_map
//
// Same names, argument meaning and ownership: the caller owns Pixels and World, the Renderer borrows them for one
// frame.  Where the reference panics these wrappers throw doom::Error carrying the dg_status code.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/doomgpu.h"

namespace doom {

struct Error : std::runtime_error {
    int code;
    Error(int c, const char *m) : std::runtime_error(m), code(c) {}
};
inline int check(int rc) { if (rc < 0) throw Error(rc, dg_last_error()); return rc; }

struct Color { uint8_t r, g, b, a; };            // sdl2::pixels::Color as the reference uses it
struct Vertex { float x, y; };                   // src/map/vertexes.rs:9-13
struct Player { Vertex position; float floor_height; float angle; };   // src/game.rs:40-45
// What the renderer reads of the game state that thinkers mutate between frames:
// floor_height / ceiling_height: what doors, lifts and crushers move; kAsLoaded (the default): the height the SECTORS lump gave.
constexpr int32_t kAsLoaded = INT32_MIN;
struct Sector { int16_t light_level; int32_t floor_height = kAsLoaded, ceiling_height = kAsLoaded; };   // src/map/sectors.rs:8-17 (src/lights.rs:47-259 writes the level)
struct State { const char *sprite; uint8_t frame; bool full_bright; bool is_null; };             // src/info.rs:1265-1273; sprite = "{:?}" of SpriteId; is_null: StateId::S_NULL
struct MapObject { State state; };                                                               // src/map_objects.rs:10-17 (MapObjectThinker :63-121 writes it)

// src/renderer/pixels.rs:5-47 with the frame size a run-time value (the reference's SCREEN_WIDTH/HEIGHT constants).
class Pixels {
public:
    std::vector<uint8_t> pixels;                 // width * height * 3, R,G,B
    int width, height;
    Pixels(int w, int h) : pixels((size_t)w * (size_t)h * 3, 0), width(w), height(h) {}
    void clear() { std::fill(pixels.begin(), pixels.end(), 0); }
    void set(size_t x, size_t y, const Color &c) {                       // pixels.rs:22-31 (y > H, not >=, as written)
        if (x >= (size_t)width || y > (size_t)height) return;
        size_t o = 3 * (y * (size_t)width + x);
        pixels.at(o) = c.r; pixels.at(o + 1) = c.g; pixels.at(o + 2) = c.b;
    }
    void draw_vertical_line(int x, int top, int bottom, const Color &c) {  // pixels.rs:33-47 (skips x <= 0)
        if (x <= 0 || x >= width) return;
        for (int y = top; y < bottom + 1; y++) {
            if (y < 0 || y >= height) continue;
            size_t o = 3 * ((size_t)y * (size_t)width + (size_t)x);
            pixels[o] = c.r; pixels[o + 1] = c.g; pixels[o + 2] = c.b;
        }
    }
};

// Everything Game::new loads besides SDL (src/game.rs:142-167).
class World {
public:
    World(const std::vector<uint8_t> &wad, const std::string &map_name) { check(dg_scene_load_wad(wad.data(), wad.size(), map_name.c_str(), &h_)); }
    ~World() { dg_scene_free(h_); }
    World(const World &) = delete;
    World &operator=(const World &) = delete;
    Player player_start() const {                                        // src/game.rs:151-156 + :376-389
        Player p{{0, 0}, 0.0f, 0.0f};
        check(dg_scene_player_start(h_, &p.position.x, &p.position.y, &p.angle));
        dg_scene_floor_height_at(h_, p.position.x, p.position.y, &p.floor_height);
        return p;
    }
    int sector_count() const { return dg_scene_sector_count(h_); }       // = map.sectors.len()
    int mobj_count() const { return dg_scene_mobj_count(h_); }           // = map_objects.objects.len()
    // Game::new, BEFORE Device::upload: decode a (sprite, frame) a later state may show (Sprites::new loads every sprite lump eagerly,
    // src/graphics/sprites.rs:26-97).  false: the WAD has no such sprite.
    bool preload_sprite_frame(const char *sprite, uint8_t frame) { return dg_scene_sprite_frame(h_, sprite, frame) >= 0; }
    // Game::new, BEFORE Device::upload: draw the animated (DG_WALL_ANIMATE) and scrolling (DG_WALL_SCROLL) walls the reference leaves
    // static.  May decode the animation frames' bitmaps.
    void set_wall_effects(uint32_t flags) { check(dg_scene_set_wall_effects(h_, flags)); }
    int wall_texture_id(const char *name, float timestamp) const { return dg_scene_wall_texture_id(h_, name, timestamp); }
    // Game::new, BEFORE Device::upload: draw the sector light effects (DG_LIGHT_THINKERS: lights.rs' thinkers as functions of the view's
    // timestamp, random ones from `seed`).  A game that runs the thinkers itself leaves this off.
    void set_light_effects(uint32_t flags, uint64_t seed) { check(dg_scene_set_light_effects(h_, flags, seed)); }
    // Every sector's level at `timestamp` as drawn with no view state (for list-path callers); out.size() sectors.
    void sector_lights_at(float timestamp, std::vector<int16_t> &out) const {
        out.resize((size_t)dg_scene_sector_count(h_));
        check(dg_scene_sector_lights_at(h_, timestamp, out.data(), (int)out.size()));
    }
    // Game::new, BEFORE Device::upload: run the map-object state machine (DG_MOBJ_THINKERS: map_objects.rs' MapObjectThinker as a
    // function of the view's timestamp) over the caller's tables — info::STATES / MAP_OBJECT_INFOS, row 0 = S_NULL.
    // A game that runs the thinkers itself leaves this off.
    void set_mobj_thinkers(uint32_t flags, const std::vector<dg_state_rec> &states, const std::vector<dg_mobj_info_rec> &infos) {
        check(dg_scene_set_mobj_thinkers(h_, flags, states.data(), (int)states.size(), infos.data(), (int)infos.size()));
    }
    // kill_everything / explode_everything / respawn_everything (DG_MOBJ_KILL, _EXPLODE, _RESPAWN) at `timestamp`; 0 clears the list.
    void mobj_event(int what, float timestamp) { check(dg_scene_mobj_event(h_, what, timestamp)); }
    // Every map object's state at `timestamp` as drawn with no view state (for list-path callers); out.size() map objects.
    void mobj_states_at(float timestamp, std::vector<dg_mobj_state> &out) const {
        out.resize((size_t)dg_scene_mobj_count(h_));
        check(dg_scene_mobj_states_at(h_, timestamp, out.data(), (int)out.size()));
    }
    // map.sectors as loaded: every sector's light level as drawn at timestamp 0 and its two heights (the start of a caller's own copy).
    std::vector<Sector> sectors() const {
        const size_t n = (size_t)dg_scene_sector_count(h_);
        std::vector<int16_t> light(n), fl(n), ce(n);
        check(dg_scene_sector_lights_at(h_, 0.0f, light.data(), (int)n));
        check(dg_scene_sector_heights(h_, fl.data(), ce.data(), (int)n));
        std::vector<Sector> out(n);
        for (size_t i = 0; i < n; i++) out[i] = Sector{light[i], fl[i], ce[i]};
        return out;
    }
    // The sectors whose heights sync_state last found moved: what Renderer::render passes as the view's entries.
    const std::vector<dg_sector_heights> &moved_sectors() const { return moved_; }
    void set_moved_sectors(const std::vector<Sector> &sectors) {
        const size_t n = (size_t)dg_scene_sector_count(h_);
        std::vector<int16_t> fl(n), ce(n);
        if (n) check(dg_scene_sector_heights(h_, fl.data(), ce.data(), (int)n));
        moved_.clear();
        for (size_t i = 0; i < sectors.size() && i < n; i++) {
            const int32_t f = sectors[i].floor_height == kAsLoaded ? fl[i] : sectors[i].floor_height;
            const int32_t c = sectors[i].ceiling_height == kAsLoaded ? ce[i] : sectors[i].ceiling_height;
            if (f != fl[i] || c != ce[i]) moved_.push_back(dg_sector_heights{(int32_t)i, f, c});
        }
    }
    // Game::new, BEFORE Device::upload: the bitmap id of a wall texture / the handle of a flat a later tick may put on a sidedef or a
    // sector (Textures::get / Flats::get_animated by name; decoded now if the map did not use it).  DG_TEX_NONE for "-".
    int use_texture(const char *name) { return std::string(name) == "-" ? DG_TEX_NONE : check(dg_scene_use_texture(h_, name)); }
    int use_flat(const char *name) { return check(dg_scene_use_flat(h_, name)); }
    // map.sidedefs' textures and offsets and map.sectors' flats as loaded (the start of a caller's own copy).
    std::vector<dg_side_surface> sidedefs() const {
        std::vector<dg_side_surface> out((size_t)dg_scene_sidedef_count(h_));
        if (!out.empty()) check(dg_scene_sidedef_surfaces(h_, out.data(), (int)out.size()));
        return out;
    }
    std::vector<dg_sector_flats> sector_flats() const {
        std::vector<dg_sector_flats> out((size_t)dg_scene_sector_count(h_));
        if (!out.empty()) check(dg_scene_sector_flats(h_, out.data(), (int)out.size()));
        return out;
    }
    // The sidedefs and sectors whose surfaces sync_surfaces last found changed: what Renderer::render passes as the view's entries
    // (DESIGN.md section 8p).
    const std::vector<dg_side_surface> &changed_sidedefs() const { return changed_sides_; }
    const std::vector<dg_sector_flats> &changed_flats() const { return changed_flats_; }
    void set_changed_surfaces(const std::vector<dg_side_surface> &sides, const std::vector<dg_sector_flats> &flats) {
        if (!loaded_known_) { loaded_sides_ = sidedefs(); loaded_flats_ = sector_flats(); loaded_known_ = true; }   // (asked once: what loaded does not change)
        const std::vector<dg_side_surface> &s0 = loaded_sides_;
        const std::vector<dg_sector_flats> &f0 = loaded_flats_;
        changed_sides_.clear(); changed_flats_.clear();
        for (size_t i = 0; i < sides.size() && i < s0.size(); i++) {
            const dg_side_surface &a = sides[i], &b = s0[i];
            if (a.tex_mid != b.tex_mid || a.tex_low != b.tex_low || a.tex_up != b.tex_up || a.x_offset != b.x_offset || a.y_offset != b.y_offset)
                changed_sides_.push_back(dg_side_surface{(int32_t)i, a.tex_mid, a.tex_low, a.tex_up, a.x_offset, a.y_offset});
        }
        for (size_t i = 0; i < flats.size() && i < f0.size(); i++)
            if (flats[i].floor_flat != f0[i].floor_flat || flats[i].ceil_flat != f0[i].ceil_flat) changed_flats_.push_back(dg_sector_flats{(int32_t)i, flats[i].floor_flat, flats[i].ceil_flat});
    }
    bool sector_floor_height(const Vertex &v, float &out) const { return dg_scene_floor_height_at(h_, v.x, v.y, &out) == 0; }  // bsp.rs:9-44
    dg_scene *handle() const { return h_; }
private:
    dg_scene *h_ = nullptr;
    std::vector<dg_sector_heights> moved_;
    std::vector<dg_side_surface> changed_sides_, loaded_sides_;
    std::vector<dg_sector_flats> changed_flats_, loaded_flats_;
    bool loaded_known_ = false;
};

// Game::render, before Renderer(..).render(): the light levels and map-object states of this tick (rust/src/gpu.rs sync_state).
// Index = position in `map.sectors` / `map_objects.objects`.  The sectors' heights that differ from the loaded ones are kept in the
// World for the next Renderer (a per-view entry each: the scene's own table does not change).
inline void sync_state(World &world, const std::vector<Sector> &sectors, const std::vector<MapObject> &objects) {
    world.set_moved_sectors(sectors);
    for (size_t i = 0; i < sectors.size(); i++) check(dg_scene_set_sector_light(world.handle(), (int)i, sectors[i].light_level));
    for (size_t i = 0; i < objects.size(); i++) {
        const State &st = objects[i].state;
        check(dg_scene_set_mobj_state(world.handle(), (int)i, st.is_null ? nullptr : st.sprite, st.frame, st.full_bright ? 1 : 0));
    }
}

// Game::render, likewise: the sidedefs' textures and offsets and the sectors' flats of this tick, index = position in `map.sidedefs` /
// `map.sectors`, each the caller's copy of World::sidedefs() / World::sector_flats() with what switches, scrollers and "change texture"
// specials did to it.  What differs from the loaded values is kept in the World for the next Renderer.
inline void sync_surfaces(World &world, const std::vector<dg_side_surface> &sides, const std::vector<dg_sector_flats> &flats) { world.set_changed_surfaces(sides, flats); }

// One GPU.  Not in the reference (it has no device); plays the role of the borrowed `&mut Pixels` target's backing store.
class Device {
public:
    Device(int width, int height, int max_batch = 1, int device = 0) {
        dg_config cfg{device, width, height, max_batch, 2, 0, DG_FE_AUTO};
        check(dg_create(&cfg, &h_));
    }
    ~Device() { dg_destroy(h_); }
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    void upload(const World &w) { check(dg_upload_scene(h_, w.handle())); }
    dg_ctx *handle() const { return h_; }
private:
    dg_ctx *h_ = nullptr;
};

// A recorded play-through moved as Game::process_down_keys + update_current_player_height move the player (src/game.rs:314-389;
// DESIGN.md section 8e): keys[t] is the DG_KEY_* mask held during tic t + 1.  locate() finds the floor heights of many walks in one
// pass on the GPU; without it floors() / players() find them on the host.  The World must outlive the Walk.
class Walk {
public:
    Walk(const World &world, const std::vector<uint8_t> &keys, int turbo = 100) {                       // from Player1Start
        dg_walk_desc d{0, 0, 0, 1, turbo, keys.data(), (uint32_t)keys.size()};
        check(dg_walk_create(world.handle(), &d, &h_));
    }
    Walk(const World &world, const Vertex &position, float angle, const std::vector<uint8_t> &keys, int turbo = 100) {   // OverridePlayer
        dg_walk_desc d{position.x, position.y, angle, 0, turbo, keys.data(), (uint32_t)keys.size()};
        check(dg_walk_create(world.handle(), &d, &h_));
    }
    ~Walk() { dg_walk_free(h_); }
    Walk(const Walk &) = delete;
    Walk &operator=(const Walk &) = delete;
    int tics() const { return dg_walk_tics(h_); }
    int probe_count() const { return dg_walk_probe_count(h_); }
    std::vector<float> floors() {
        std::vector<float> out((size_t)tics() + 1);
        check(dg_walk_floors(h_, out.data(), (int)out.size()));
        return out;
    }
    // The views at these timestamps, ready for dg_render_views / dg_submit_views / dg_render_map_views.
    std::vector<dg_view> views(const std::vector<float> &timestamps) {
        std::vector<dg_view> out(timestamps.size());
        check(dg_walk_views(h_, timestamps.data(), (int)timestamps.size(), out.data()));
        return out;
    }
    static void locate(Device &dev, const std::vector<Walk *> &walks) {
        std::vector<dg_walk *> hs;
        for (Walk *w : walks) hs.push_back(w->h_);
        check(dg_ctx_locate_walks(dev.handle(), hs.data(), (int)hs.size()));
    }
private:
    dg_walk *h_ = nullptr;
};

// src/renderer/mod.rs:27-58,118-136: construct per frame, call render(), read pixels.pixels.
class Renderer {
public:
    Renderer(Pixels &pixels, const World &world, const Player &player, float timestamp, Device &dev)
        : pixels_(pixels), dev_(dev), world_(world) {
        // (the device already holds the uploaded world; what the Renderer reads of it are the sector heights sync_state found moved)
        // Vertex::rotate (src/map/vertexes.rs:20-25) evaluates f32::cos / f32::sin of +-angle: the same libm calls, made here,
        // so that the library consumes the caller's bits (trig_valid = 1) instead of evaluating its own
        const float a = player.angle;
        view_ = dg_view{player.position.x, player.position.y, a, player.floor_height, std::cos(a), std::sin(a), std::cos(-a), std::sin(-a), timestamp, 1};
    }
    void render() {
        const std::vector<dg_sector_heights> &moved = world_.moved_sectors();
        const dg_view_sectors vs{moved.data(), (uint32_t)moved.size()};
        const std::vector<dg_side_surface> &sides = world_.changed_sidedefs();
        const std::vector<dg_sector_flats> &flats = world_.changed_flats();
        const dg_view_surfaces vf{sides.data(), (uint32_t)sides.size(), flats.data(), (uint32_t)flats.size()};
        check(dg_render_views_surfaces(dev_.handle(), &view_, nullptr, nullptr, moved.empty() ? nullptr : &vs, sides.empty() && flats.empty() ? nullptr : &vf, 1, pixels_.pixels.data()));
    }
    // The viewing_map branch of Game::render (src/game.rs:491-499): canvas.clear() to black, draw_map_linedefs, draw_map_player, into
    // the same Pixels.  Reads the player's position and angle only.
    void render_map() { check(dg_render_map_views(dev_.handle(), &view_, 1, pixels_.pixels.data())); }
private:
    Pixels &pixels_;
    Device &dev_;
    const World &world_;
    dg_view view_;
};

}  // namespace doom
