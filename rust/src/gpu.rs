//! gpu.rs — FFI binding of libdoomgpu (include/doomgpu.h) for freewilll/doom-rust-renderer.
//!
//! Drop this file into the reference crate as `src/renderer/gpu.rs`, add `pub mod gpu;` to `src/renderer/mod.rs`, put
//! `rust/build.rs` next to the crate's Cargo.toml and apply the three edits to `src/game.rs` described in rust/README.md.
//! UNBUILT in this repository: the build image has no rustc / cargo.  The C++ mirror of the same interface
//! (doom-rust-renderer_amd/csrc/doomgpu.hpp) and the ctypes binding are the ones the test tiers execute.
#![allow(non_camel_case_types)]
use std::ffi::{c_char, c_int, c_void, CStr, CString};

#[repr(C)] pub struct dg_scene { _p: [u8; 0] }
#[repr(C)] pub struct dg_ctx   { _p: [u8; 0] }

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct dg_view {                       // Player (src/game.rs:40-45) + Renderer::new's timestamp
    pub x: f32, pub y: f32, pub angle: f32, pub floor_height: f32,
    pub cos_a: f32, pub sin_a: f32, pub cos_na: f32, pub sin_na: f32,
    pub timestamp: f32, pub trig_valid: i32,
}
#[repr(C)]
pub struct dg_config { pub device: i32, pub width: i32, pub height: i32, pub max_batch: i32, pub slots: i32, pub host_threads: i32, pub front_end: i32 }

#[repr(C)] #[derive(Clone, Copy)]
pub struct dg_bitmap_column { pub x: i16, pub clipped_top_y: i16, pub clipped_bottom_y: i16, pub bottom_y: i16, pub top_y: i16 } // bitmap_render.rs:19-25
#[repr(C)] #[derive(Clone, Copy)]
pub struct dg_bitmap_render {              // bitmap_render.rs:29-45
    pub bitmap: i32, pub light_level: i16, pub offset_x: i16, pub offset_y: i16, pub reserved: i16,
    pub line_start_x: f32, pub line_start_y: f32, pub line_end_x: f32, pub line_end_y: f32, pub start_offset: f32,
    pub start_x: i32, pub end_x: i32, pub bottom_height: f32, pub top_height: f32,
    pub first_column: u32, pub n_columns: u32,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct dg_visplane { pub flat: i32, pub height: i16, pub light_level: i16, pub left: i16, pub right: i16, pub first_entry: u32 } // visplanes.rs:17-26
#[repr(C)] #[derive(Clone, Copy)]
pub struct dg_draw_cmd { pub kind: u32, pub index: u32 }
#[repr(C)]
pub struct dg_frame_lists {
    pub view: dg_view,
    pub renders: *const dg_bitmap_render, pub n_renders: u32,
    pub columns: *const dg_bitmap_column, pub n_columns: u32,
    pub visplanes: *const dg_visplane,    pub n_visplanes: u32,
    pub plane_tb: *const i16,             pub n_plane_tb: u32,
    pub order: *const dg_draw_cmd,        pub n_order: u32,
}

/// One line of a 2-D map frame (dg_map_lines): rgb = r | g << 8 | b << 16.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct dg_map_line { pub x0: i32, pub y0: i32, pub x1: i32, pub y1: i32, pub rgb: u32 }
/// Box downscale of a reduced readback (dg_readback_reduced): fx, fy in 1..16, format 0 = RGB24, 1 = GRAY8.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct dg_reduce_desc { pub fx: u32, pub fy: u32, pub format: u32, pub reserved: u32 }
pub const DG_FE_MAP: i32 = 4;              // dg_timing.front_end of a map submission
pub const DG_WALL_ANIMATE: u32 = 1;         // dg_scene_set_wall_effects flags
pub const DG_WALL_SCROLL: u32 = 2;
pub const DG_LIGHT_THINKERS: u32 = 1;       // dg_scene_set_light_effects flag
pub const DG_MOBJ_THINKERS: u32 = 1;        // dg_scene_set_mobj_thinkers flag
pub const DG_MOBJ_KILL: c_int = 1;          // dg_scene_mobj_event
pub const DG_MOBJ_EXPLODE: c_int = 2;
pub const DG_MOBJ_RESPAWN: c_int = 3;
#[repr(C)]
#[derive(Clone, Copy)]
pub struct dg_state_rec { pub sprite: [u8; 4], pub frame: u8, pub full_bright: u8, pub tics: i16, pub next_state: i32 }
#[repr(C)]
#[derive(Clone, Copy)]
pub struct dg_mobj_info_rec { pub doomednum: i32, pub spawn_state: i32, pub death_state: i32, pub xdeath_state: i32 }

extern "C" {
    pub fn dg_scene_load_wad(wad: *const u8, len: usize, map_name: *const c_char, out: *mut *mut dg_scene) -> c_int;
    pub fn dg_scene_free(s: *mut dg_scene);
    pub fn dg_scene_player_start(s: *const dg_scene, x: *mut f32, y: *mut f32, angle: *mut f32) -> c_int;
    pub fn dg_scene_floor_height_at(s: *const dg_scene, x: f32, y: f32, h: *mut f32) -> c_int;
    pub fn dg_scene_set_sector_light(s: *mut dg_scene, sector: c_int, light: i16) -> c_int;
    pub fn dg_scene_set_mobj_state(s: *mut dg_scene, mobj: c_int, sprite: *const c_char, frame: u8, full_bright: c_int) -> c_int;
    pub fn dg_scene_texture_id(s: *const dg_scene, name: *const c_char) -> c_int;
    pub fn dg_scene_flat_id(s: *const dg_scene, name: *const c_char, timestamp: f32) -> c_int;
    pub fn dg_scene_set_wall_effects(s: *mut dg_scene, flags: u32) -> c_int;
    pub fn dg_scene_wall_texture_id(s: *const dg_scene, name: *const c_char, timestamp: f32) -> c_int;
    pub fn dg_scene_set_light_effects(s: *mut dg_scene, flags: u32, seed: u64) -> c_int;
    pub fn dg_scene_sector_lights_at(s: *const dg_scene, timestamp: f32, out: *mut i16, n: c_int) -> c_int;
    pub fn dg_scene_set_mobj_thinkers(s: *mut dg_scene, flags: u32, states: *const dg_state_rec, n_states: c_int,
                                      infos: *const dg_mobj_info_rec, n_infos: c_int) -> c_int;
    pub fn dg_scene_mobj_event(s: *mut dg_scene, what: c_int, timestamp: f32) -> c_int;
    pub fn dg_scene_mobj_states_at(s: *const dg_scene, timestamp: f32, out: *mut dg_mobj_state, n: c_int) -> c_int;
    pub fn dg_scene_sprite_bitmap_id(s: *const dg_scene, sprite: *const c_char, frame: u8, rotation: u8) -> c_int;
    pub fn dg_scene_sprite_frame(s: *mut dg_scene, sprite: *const c_char, frame: u8) -> c_int;
    pub fn dg_scene_sector_count(s: *const dg_scene) -> c_int;
    pub fn dg_scene_mobj_count(s: *const dg_scene) -> c_int;
    pub fn dg_create(cfg: *const dg_config, out: *mut *mut dg_ctx) -> c_int;
    pub fn dg_destroy(ctx: *mut dg_ctx);
    pub fn dg_upload_scene(ctx: *mut dg_ctx, scene: *const dg_scene) -> c_int;
    pub fn dg_render_views(ctx: *mut dg_ctx, views: *const dg_view, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_draw_lists(ctx: *mut dg_ctx, slot: c_int, frames: *const dg_frame_lists, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_frame_checksums(ctx: *mut dg_ctx, slot: c_int, first: c_int, count: c_int, out: *mut u64) -> c_int;
    pub fn dg_readback_reduced(ctx: *mut dg_ctx, slot: c_int, first: c_int, count: c_int, desc: *const dg_reduce_desc, dst_host: *mut u8) -> c_int;
    pub fn dg_map_lines(s: *const dg_scene, width: c_int, height: c_int, view: *const dg_view, out: *mut dg_map_line, cap: c_int) -> c_int;
    pub fn dg_submit_map_views(ctx: *mut dg_ctx, slot: c_int, views: *const dg_view, n: c_int) -> c_int;
    pub fn dg_render_map_views(ctx: *mut dg_ctx, views: *const dg_view, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_last_error() -> *const c_char;
}

/// Drop-in for `Renderer`: same life cycle as src/renderer/mod.rs:37-58,118-136 (built per frame, borrows Pixels).
pub struct GpuRenderer<'a> { ctx: *mut dg_ctx, pixels: &'a mut super::Pixels, view: dg_view, poses: Vec<dg_mobj_pose>, sectors: Vec<dg_sector_heights> }

impl<'a> GpuRenderer<'a> {
    pub fn new(ctx: *mut dg_ctx, pixels: &'a mut super::Pixels, player: &crate::game::Player, timestamp: f32) -> Self {
        let a = player.angle;
        GpuRenderer { ctx, pixels, view: dg_view {
            x: player.position.x, y: player.position.y, angle: a, floor_height: player.floor_height,
            cos_a: a.cos(), sin_a: a.sin(), cos_na: (-a).cos(), sin_na: (-a).sin(),   // what Vertex::rotate computes (vertexes.rs:20-25)
            timestamp, trig_valid: 1 }, poses: Vec::new(), sectors: Vec::new() }
    }
    /// Where this tick's map objects are (what `sync_state` returned): without it every object stands where the THINGS lump put it.
    pub fn with_poses(mut self, poses: Vec<dg_mobj_pose>) -> Self { self.poses = poses; self }
    /// This tick's sector heights (what `sector_heights` returned): without it every floor and ceiling stands as the SECTORS lump loaded it.
    pub fn with_sectors(mut self, sectors: Vec<dg_sector_heights>) -> Self { self.sectors = sectors; self }
    pub fn render(&mut self) {
        let vp = dg_view_poses { poses: self.poses.as_ptr(), n: self.poses.len() as u32 };
        let vs = dg_view_sectors { heights: self.sectors.as_ptr(), n: self.sectors.len() as u32 };
        let rc = unsafe { dg_render_views_sectors(self.ctx, &self.view, std::ptr::null(), &vp, &vs, 1, self.pixels.pixels.as_mut_ptr()) };
        if rc != 0 { panic!("doomgpu: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }  // the reference panics too
    }
    /// The `viewing_map` branch of Game::render (src/game.rs:491-499): black, draw_map_linedefs, draw_map_player — into the same
    /// Pixels, so the caller copies `pixels.pixels` into the window texture as for a 3-D frame and needs no SDL canvas path.
    pub fn render_map(&mut self) {
        let rc = unsafe { dg_render_map_views(self.ctx, &self.view, 1, self.pixels.pixels.as_mut_ptr()) };
        if rc != 0 { panic!("doomgpu: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
    }
}

// ---- live game state: what the thinkers changed since the last frame ------------------------------------------------------------
// The renderer reads `sector.light_level` (src/renderer/segs.rs:450-455 via the sector, mutated by src/lights.rs:47-259) and
// `map_object.state` (src/renderer/map_objects.rs:34-70, mutated by MapObjectThinker, src/map_objects.rs:63-121) every frame.  The
// library keeps its own copy of both inside dg_scene; sync_state() copies the game's current values into it.  Indices are positions
// in `map.sectors` / `map_objects.objects`, which is how doom-rust-renderer_amd/csrc/scene.cpp numbers them (sectors in lump order,
// src/map/sectors.rs:20-41; map objects = THINGS minus the player / deathmatch starts, src/map_objects.rs:25-50).

/// `Game::new`, BEFORE dg_upload_scene: decode every (sprite, frame) a state can show — what `Sprites::new` does eagerly
/// (src/graphics/sprites.rs:26-97) — so that no later `sync_state` meets a bitmap the GPU does not hold.  Sprites the WAD lacks
/// (shareware IWADs) are skipped exactly like `Sprites::get_picture` would only fail when such a state is drawn.
/// Game::new, before dg_upload_scene: draw animated (SLADRIP, BFALL, ...) and scrolling (linedef special 48) walls, which the
/// reference renders static.  `flags`: DG_WALL_ANIMATE | DG_WALL_SCROLL, or 0.
pub fn set_wall_effects(scene: *mut dg_scene, flags: u32) {
    let rc = unsafe { dg_scene_set_wall_effects(scene, flags) };
    if rc < 0 { panic!("dg_scene_set_wall_effects: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
}

/// Game::new, before dg_upload_scene: draw the sector light effects (flicker, strobes, glow, fire: lights.rs) as functions of the
/// timestamp, for callers that run no thinkers.  A game that runs `init_thinkers` itself keeps `sync_state` and leaves this off.
pub fn set_light_effects(scene: *mut dg_scene, flags: u32, seed: u64) {
    let rc = unsafe { dg_scene_set_light_effects(scene, flags, seed) };
    if rc < 0 { panic!("dg_scene_set_light_effects: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
}

/// Game::new, before dg_upload_scene: let the library run the map-object state machine (map_objects.rs:62-121) as a function of the
/// timestamp, for callers that run no thinkers.  The tables are info::STATES / MAP_OBJECT_INFOS as they stand: StateId values are the
/// rows' indices (S_NULL = 0).  A game that runs `init_thinkers` itself keeps `sync_state` and leaves this off.
pub fn set_mobj_thinkers(scene: *mut dg_scene, flags: u32) {
    let states: Vec<dg_state_rec> = crate::info::STATES.iter().map(|st| {
        let name = format!("{:?}", st.sprite);
        let mut sprite = [0u8; 4];
        for (d, b) in sprite.iter_mut().zip(name.bytes()) { *d = b; }
        dg_state_rec { sprite, frame: st.frame, full_bright: st.full_bright as u8, tics: st.tics, next_state: st.next_state as i32 }
    }).collect();
    let infos: Vec<dg_mobj_info_rec> = crate::info::MAP_OBJECT_INFOS.iter().map(|i| dg_mobj_info_rec {
        doomednum: i.id as i32, spawn_state: i.spawn_state as i32, death_state: i.death_state as i32, xdeath_state: i.xdeath_state as i32,
    }).collect();
    let rc = unsafe { dg_scene_set_mobj_thinkers(scene, flags, states.as_ptr(), states.len() as c_int, infos.as_ptr(), infos.len() as c_int) };
    if rc < 0 { panic!("dg_scene_set_mobj_thinkers: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
}

/// The K / X / R keys (kill_everything, explode_everything, respawn_everything) at `timestamp`; takes effect at the next dg_upload_scene.
pub fn mobj_event(scene: *mut dg_scene, what: c_int, timestamp: f32) {
    let rc = unsafe { dg_scene_mobj_event(scene, what, timestamp) };
    if rc < 0 { panic!("dg_scene_mobj_event: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
}

pub fn preload_sprite_frames(scene: *mut dg_scene) {
    for st in crate::info::STATES.iter() {
        let name = CString::new(format!("{:?}", st.sprite)).unwrap();          // the lump prefix Sprites::new matches on (sprites.rs:30)
        unsafe { dg_scene_sprite_frame(scene, name.as_ptr(), st.frame) };     // < 0: not in this WAD
    }
}

/// `Game::render`, before `GpuRenderer::new(..).render()`: push the light levels and map-object states of this tick, and return where
/// the map objects are.  Light levels and states live in the scene; positions and angles travel per view (dg_view_poses, DESIGN.md
/// section 8m) — `MapObject.position` / `.angle` are what draw_map_objects reads on every frame (src/renderer/map_objects.rs:55,74), and
/// the library derives the sector, hence light and z, from the position as the reference does (:99-116).
pub fn sync_state(scene: *mut dg_scene, map: &crate::map::Map, map_objects: &crate::map_objects::MapObjects) -> Vec<dg_mobj_pose> {
    for (i, sector) in map.sectors.iter().enumerate() {
        let rc = unsafe { dg_scene_set_sector_light(scene, i as c_int, sector.borrow().light_level) };
        if rc != 0 { panic!("doomgpu: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
    }
    for (i, object) in map_objects.objects.iter().enumerate() {
        let o = object.borrow();
        let rc = if o.state.id == crate::info::StateId::S_NULL {               // not drawn (renderer/map_objects.rs:37)
            unsafe { dg_scene_set_mobj_state(scene, i as c_int, std::ptr::null(), 0, 0) }
        } else {
            let name = CString::new(format!("{:?}", o.state.sprite)).unwrap();
            unsafe { dg_scene_set_mobj_state(scene, i as c_int, name.as_ptr(), o.state.frame, o.state.full_bright as c_int) }
        };
        if rc != 0 { panic!("doomgpu: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
    }
    map_objects.objects.iter().enumerate().map(|(i, object)| {
        let o = object.borrow();
        dg_mobj_pose { mobj: i as i32, x: o.position.x, y: o.position.y, angle: o.angle }
    }).collect()
}

// ---- per-view map-object poses (include/doomgpu.h dg_view_poses): MapObject.position / .angle of ONE view ---------------
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_mobj_pose { pub mobj: i32, pub x: f32, pub y: f32, pub angle: f32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_view_poses { pub poses: *const dg_mobj_pose, pub n: u32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_mobj_placed { pub x: f32, pub y: f32, pub angle: f32, pub sector: i32 }
extern "C" {
    pub fn dg_render_views_poses(ctx: *mut dg_ctx, views: *const dg_view, states: *const dg_view_state, poses: *const dg_view_poses, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_submit_views_poses(ctx: *mut dg_ctx, slot: c_int, views: *const dg_view, states: *const dg_view_state, poses: *const dg_view_poses, n: c_int) -> c_int;
    pub fn dg_slot_mobj_poses(ctx: *mut dg_ctx, slot: c_int, first: c_int, count: c_int, out: *mut dg_mobj_placed) -> c_int;
}

// ---- per-view sector heights (include/doomgpu.h dg_view_sectors): Sector.floor_height / .ceiling_height of ONE view ----
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_sector_heights { pub sector: i32, pub floor_height: i32, pub ceiling_height: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_view_sectors { pub heights: *const dg_sector_heights, pub n: u32 }
extern "C" {
    pub fn dg_render_views_sectors(ctx: *mut dg_ctx, views: *const dg_view, states: *const dg_view_state, poses: *const dg_view_poses, sectors: *const dg_view_sectors, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_submit_views_sectors(ctx: *mut dg_ctx, slot: c_int, views: *const dg_view, states: *const dg_view_state, poses: *const dg_view_poses, sectors: *const dg_view_sectors, n: c_int) -> c_int;
    pub fn dg_scene_sector_heights(scene: *const dg_scene, floor: *mut i16, ceiling: *mut i16, n: c_int) -> c_int;
    pub fn dg_slot_sector_heights(ctx: *mut dg_ctx, slot: c_int, first: c_int, count: c_int, out: *mut i16) -> c_int;
}
/// `Game::render`, next to `sync_state`: every sector's current heights as the view's entries — doors, lifts and
/// crushers move `Sector.floor_height` / `.ceiling_height`, which process_seg reads on every frame (src/renderer/segs.rs:376-402).
/// An entry equal to the loaded heights changes nothing, so all sectors may be sent; the heights are i16 in the reference.
pub fn sector_heights(map: &crate::map::Map) -> Vec<dg_sector_heights> {
    map.sectors.iter().enumerate().map(|(i, sector)| {
        let s = sector.borrow();
        dg_sector_heights { sector: i as i32, floor_height: s.floor_height as i32, ceiling_height: s.ceiling_height as i32 }
    }).collect()
}

// ---- per-view game state (include/doomgpu.h dg_view_state): what the thinkers changed before a frame ------------------
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_sector_light { pub sector: i32, pub light_level: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct dg_mobj_state { pub mobj: i32, pub sprite_frame: i32, pub full_bright: i32, pub reserved: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct dg_view_state { pub lights: *const dg_sector_light, pub n_lights: u32, pub mobjs: *const dg_mobj_state, pub n_mobjs: u32 }
extern "C" {
    pub fn dg_render_views_state(ctx: *mut dg_ctx, views: *const dg_view, states: *const dg_view_state, n: c_int, rgb24_out: *mut u8) -> c_int;
    pub fn dg_submit_views_state(ctx: *mut dg_ctx, slot: c_int, views: *const dg_view, states: *const dg_view_state, n: c_int) -> c_int;
    pub fn dg_wait(ctx: *mut dg_ctx, slot: c_int) -> c_int;
    pub fn dg_readback_async(ctx: *mut dg_ctx, slot: c_int, first: c_int, count: c_int, rgb24_out: *mut u8) -> c_int;
}

// ---- player movement from recorded keys (include/doomgpu.h dg_walk_*) ----------------------------------------
// A replayed play-through: what Game::process_down_keys and update_current_player_height (src/game.rs:314-389) do to the player, tic
// by tic, from one key mask per tic.  dg_ctx_locate_walks finds the floor heights of many walks in one pass on the GPU.
pub const DG_KEY_LEFT: u8 = 1;
pub const DG_KEY_RIGHT: u8 = 2;
pub const DG_KEY_UP: u8 = 4;
pub const DG_KEY_DOWN: u8 = 8;
pub const DG_KEY_ALT: u8 = 16;              // either Alt
pub const DG_KEY_SHIFT: u8 = 32;            // either Shift
#[repr(C)] pub struct dg_walk { _p: [u8; 0] }
#[repr(C)]
pub struct dg_walk_desc { pub x: f32, pub y: f32, pub angle: f32, pub from_player_start: i32, pub turbo: i32, pub keys: *const u8, pub n_tics: u32 }
extern "C" {
    pub fn dg_walk_create(s: *const dg_scene, d: *const dg_walk_desc, out: *mut *mut dg_walk) -> c_int;
    pub fn dg_walk_free(w: *mut dg_walk);
    pub fn dg_walk_tics(w: *const dg_walk) -> c_int;
    pub fn dg_walk_probe_count(w: *const dg_walk) -> c_int;
    pub fn dg_walk_floors(w: *mut dg_walk, out: *mut f32, n: c_int) -> c_int;
    pub fn dg_walk_views(w: *mut dg_walk, timestamps: *const f32, n: c_int, out: *mut dg_view) -> c_int;
    pub fn dg_ctx_locate_walks(ctx: *mut dg_ctx, walks: *const *mut dg_walk, n_walks: c_int) -> c_int;
}

/// The mask of `Game::pressed_keys` for one tic (src/game.rs:319-372).
pub fn key_mask(pressed: &std::collections::HashSet<sdl2::keyboard::Keycode>) -> u8 {
    use sdl2::keyboard::Keycode as K;
    let has = |k: K| pressed.contains(&k);
    (has(K::Left) as u8) * DG_KEY_LEFT | (has(K::Right) as u8) * DG_KEY_RIGHT | (has(K::Up) as u8) * DG_KEY_UP | (has(K::Down) as u8) * DG_KEY_DOWN
        | ((has(K::LAlt) || has(K::RAlt)) as u8) * DG_KEY_ALT | ((has(K::LShift) || has(K::RShift)) as u8) * DG_KEY_SHIFT
}

/// A recorded play-through from Player1Start; `views` gives the dg_view of every timestamp asked for.
pub struct Walk { h: *mut dg_walk }
impl Walk {
    pub fn from_player_start(scene: *const dg_scene, turbo: i16, keys: &[u8]) -> Walk {
        let d = dg_walk_desc { x: 0.0, y: 0.0, angle: 0.0, from_player_start: 1, turbo: turbo as i32, keys: keys.as_ptr(), n_tics: keys.len() as u32 };
        let mut h = std::ptr::null_mut();
        let rc = unsafe { dg_walk_create(scene, &d, &mut h) };
        if rc != 0 { panic!("dg_walk_create: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
        Walk { h }
    }
    pub fn locate(ctx: *mut dg_ctx, walks: &[&Walk]) {
        let hs: Vec<*mut dg_walk> = walks.iter().map(|w| w.h).collect();
        let rc = unsafe { dg_ctx_locate_walks(ctx, hs.as_ptr(), hs.len() as c_int) };
        if rc != 0 { panic!("dg_ctx_locate_walks: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
    }
    pub fn views(&mut self, timestamps: &[f32]) -> Vec<dg_view> {
        let mut out = vec![dg_view::default(); timestamps.len()];
        let rc = unsafe { dg_walk_views(self.h, timestamps.as_ptr(), timestamps.len() as c_int, out.as_mut_ptr()) };
        if rc != 0 { panic!("dg_walk_views: {}", unsafe { CStr::from_ptr(dg_last_error()) }.to_string_lossy()); }
        out
    }
}
impl Drop for Walk { fn drop(&mut self) { unsafe { dg_walk_free(self.h) } } }
