/* doomgpu.h — C-ABI of libdoomgpu: an MI355X (gfx950) column/span rasteriser that is a drop-in for the
 * `src/renderer` hot path of freewilll/doom-rust-renderer (reference paths below are relative to that repo).
 *
 * What it replaces.  In the reference, `Game::render` (src/game.rs:491-534) does, once per frame:
 *     let mut pixels = Pixels::new();                                  // src/renderer/pixels.rs:10-14
 *     Renderer::new(&mut pixels, &map, &map_objects, &mut textures, &mut sprites, sky_texture,
 *                   &mut flats, &palette, &player, timestamp).render(); // src/renderer/mod.rs:37-58,118-136
 *     buffer.copy_from_slice(pixels.pixels.as_ref());                  // RGB24, src/game.rs:521-525
 * This library produces byte-identical `pixels.pixels` (3*W*H bytes, R,G,B, row-major) for a batch of
 * viewpoints at once, with every per-pixel evaluation done by hand-written HIP kernels.
 *
 * Two entry levels:
 *   dg_render_views  — full path: the library walks the BSP / builds the seg, visplane and sprite lists
 *                      itself (host C++, multi-threaded over frames) and rasterises them on the GPU.
 *   dg_draw_lists    — list path: the caller (e.g. the Rust host, keeping its own src/renderer/segs.rs walk)
 *                      hands over the recorded BitmapRender / Visplane lists in draw order; the library only
 *                      rasterises.  Record layouts mirror src/renderer/bitmap_render.rs:19-45 and
 *                      src/renderer/visplanes.rs:17-26.
 *
 * Conventions: every function returns 0 on success or a negative dg_status; nothing unwinds across the
 * boundary (the reference panics instead: e.g. src/renderer/segs.rs:103-111,140-145,431-436).  One dg_ctx per
 * GPU; a ctx is not thread-safe, different ctxs are independent.  There is no CPU fallback: dg_create fails
 * when no gfx950 device is present.
 */
#ifndef DOOMGPU_H
#define DOOMGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum dg_status {
    DG_OK = 0,
    DG_ERR_INVALID = -1,     /* bad argument */
    DG_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture */
    DG_ERR_HIP = -3,         /* HIP runtime error, see dg_last_error */
    DG_ERR_WAD = -4,         /* WAD/map parse error (reference: panic in src/wad.rs, src/map/, src/graphics/) */
    DG_ERR_RENDER = -5,      /* a condition on which the reference renderer panics */
    DG_ERR_CAPACITY = -6,    /* batch / list larger than the ctx was created for */
    DG_ERR_STATE = -7        /* the slot does not hold what the call reads (dg_slot_mobj_poses) */
} dg_status;

typedef struct dg_scene dg_scene; /* host-side immutable world: Map + Palette + Textures + Flats + Sprites + MapObjects */
typedef struct dg_ctx dg_ctx;     /* one GPU: device copy of a scene, staging rings, streams */

/* ---- scene (reference: Game::new minus SDL, src/game.rs:142-167) ------------------------------------------ */
/* WadFile::new + Map::new + Palette/Flats/Textures/Sprites/MapObjects::new + get_sky_texture.
 * `wad` is copied.  map_name as given to `--map` (src/main.rs:33-35), e.g. "e1m1". */
int dg_scene_load_wad(const uint8_t *wad, size_t len, const char *map_name, dg_scene **out);
void dg_scene_free(dg_scene *s);
/* Player1Start (src/game.rs:151-156). */
int dg_scene_player_start(const dg_scene *s, float *x, float *y, float *angle);
/* get_sector_from_vertex(..).floor_height (src/renderer/bsp.rs:9-44, src/game.rs:386-388).
 * Returns DG_OK and writes *floor_height, or 1 if the point is in no sector (value untouched). */
int dg_scene_floor_height_at(const dg_scene *s, float x, float y, float *floor_height);
/* Per-frame game-state snapshot hooks (the reference mutates these between frames: src/lights.rs,
 * src/map_objects.rs:63-121).  Not needed for frame-0 parity. */
int dg_scene_sector_count(const dg_scene *s);
int dg_scene_set_sector_light(dg_scene *s, int sector, int16_t light_level);
int dg_scene_mobj_count(const dg_scene *s);
/* state: sprite name (4 chars), frame (0 = 'A'), full_bright, or sprite == NULL for StateId::S_NULL (not drawn). */
int dg_scene_set_mobj_state(dg_scene *s, int mobj, const char *sprite, uint8_t frame, int full_bright);
/* A state change may decode sprite bitmaps the GPU copy does not hold yet: submissions then fail with DG_ERR_INVALID until
 * dg_upload_scene is called again (light levels never need a re-upload). */

/* Wall effects (opt-in per scene; the reference draws these walls static — DESIGN.md section 8b).  Both are functions of the view's
 * timestamp, nothing else:
 *   DG_WALL_ANIMATE  a sidedef texture (upper, lower, middle, masked middles too) that belongs to a live animated-wall list (SLADRIP1-3,
 *                    BFALL1-4, ...; live: every member is a known texture) draws list[c % n], c = the saturating u64 of timestamp * 3.0f
 *                    (NaN or <= 0: 0) — the animated-flat rule; the phase does not depend on which member the map names.
 *   DG_WALL_SCROLL   a sidedef that is the front of k linedefs of special 48 has its x offset moved by (u32)(k * tics) mod 65536,
 *                    tics = (timestamp * 35.0f) as u32 (saturating, NaN: 0), wrapped to i16.
 * Every front end gives the same pixels; the 2-D map view and dg_draw_lists ignore the flags. */
#define DG_WALL_ANIMATE 1u
#define DG_WALL_SCROLL  2u
/* Takes effect at the next dg_upload_scene; dg_build_lists sees it at once.  May decode bitmaps.  Unknown bits: DG_ERR_INVALID. */
int dg_scene_set_wall_effects(dg_scene *s, uint32_t flags);
/* The dg_scene_texture_id of `name`, after animation at `timestamp` when DG_WALL_ANIMATE is set (the dg_scene_flat_id twin, for list-path callers). */
int dg_scene_wall_texture_id(const dg_scene *s, const char *name, float timestamp);

/* Sector light effects (opt-in per scene; the reference runs them as sector thinkers, src/lights.rs — DESIGN.md section 8c).
 *   DG_LIGHT_THINKERS  every sector of special 1, 2, 3, 4, 8, 12, 13 or 17 draws the level its thinker leaves after
 *                      tics = (timestamp * 35.0f) as u32 (saturating, NaN: 0) calls of mutate(), min / max taken from the WAD's levels.
 *                      Glow (8) and the synced strobes (12, 13) equal the reference; the random draws of 1, 2, 3, 4 and 17 come from
 *                      a pinned stream of `seed` (same rules, same distributions, reproducible).
 * Per view and sector: a dg_view_state entry wins, else the effect's level, else the scene's level (dg_scene_set_sector_light).
 * Every front end gives the same pixels; the 2-D map view and dg_draw_lists ignore the flags. */
#define DG_LIGHT_THINKERS 1u
/* Takes effect at the next dg_upload_scene; dg_build_lists and dg_scene_sector_lights_at see it at once.
 * Unknown bits or a NULL scene: DG_ERR_INVALID.  flags 0 turns the effects off again. */
int dg_scene_set_light_effects(dg_scene *s, uint32_t flags, uint64_t seed);
/* The level of every sector at `timestamp` as this library draws it with no view state: the effect's level for a sector that
 * has one, else the scene's level (dg_scene_set_sector_light).  n must equal dg_scene_sector_count. */
int dg_scene_sector_lights_at(const dg_scene *s, float timestamp, int16_t *out, int n);

/* ---- viewpoint (reference: `Player`, src/game.rs:40-45, + Renderer::new's timestamp) ------------------------ */
typedef struct dg_view {
    float x, y;          /* player.position */
    float angle;         /* player.angle (radians) */
    float floor_height;  /* player.floor_height */
    float cos_a, sin_a;  /* f32::cos/sin(angle)   as the host libm returns them (src/map/vertexes.rs:20-25) */
    float cos_na, sin_na;/* f32::cos/sin(-angle) */
    float timestamp;     /* clock.timestamp: selects the animated-flat frame (src/graphics/flats.rs:103-111) and the wall effects' frame */
    int32_t trig_valid;  /* 0: the library fills the four trig fields with cosf/sinf */
} dg_view;

/* Game state of ONE view on top of the scene's: what the reference's thinkers changed before that frame was drawn — sector
 * light levels (LightFlash / StrobeFlash / GlowingLight / FireFlicker, src/lights.rs:47-259) and map-object states
 * (src/map_objects.rs:63-121).  Entries override the scene's value for that view only, so the frames of a recorded play-through
 * can travel in one batch.  sprite_frame: dg_scene_sprite_frame(), or -1 for StateId::S_NULL (not drawn). */
typedef struct dg_sector_light { int32_t sector; int32_t light_level; } dg_sector_light;
typedef struct dg_mobj_state { int32_t mobj; int32_t sprite_frame; int32_t full_bright; int32_t reserved; } dg_mobj_state;
typedef struct dg_view_state {
    const dg_sector_light *lights; uint32_t n_lights;
    const dg_mobj_state *mobjs;    uint32_t n_mobjs;
} dg_view_state;
/* Handle of (sprite, frame) for dg_mobj_state (Sprites::get_picture's first two arguments, src/graphics/sprites.rs:99-117);
 * negative on error.  Like dg_scene_set_mobj_state it may decode new bitmaps: call it before dg_upload_scene. */
int dg_scene_sprite_frame(dg_scene *s, const char *sprite, uint8_t frame);

/* Map-object state machine (opt-in per scene; the reference runs it as MapObjectThinker, src/map_objects.rs:62-121 — DESIGN.md
 * section 8d).  The state table is the CALLER's (the reference's info::STATES / MAP_OBJECT_INFOS, or a mod's): the library ships none.
 *   dg_state_rec      one state: sprite (4 characters, not terminated), frame (0 = 'A'), full_bright, tics (-1: for ever, 0: one
 *                     tic, n: n tics), next_state.  Row 0 is S_NULL: an object in it is not drawn.  `action` is not used (nor by the reference).
 *   dg_mobj_info_rec  one thing type: doomednum and its spawn, death and xdeath states.  A later row of the same doomednum wins.
 *   DG_MOBJ_THINKERS  every map object whose type has a row and whose spawn chain is live is drawn in the state its thinker shows after
 *                     tics = (timestamp * 35.0f) as u32 (saturating, NaN and <= 0: 0) calls of mutate(), the scene's events in between.
 * A chain is every state reachable from a start state through next_state; it is live when each of its states other than row 0
 * resolves as dg_scene_sprite_frame would.  An object without a row or a live spawn chain is drawn as without the setting.
 * Per view and object: a dg_view_state entry wins, else the thinker's state, else the scene's (dg_scene_set_mobj_state).
 * Every front end gives the same pixels; the 2-D map view and dg_draw_lists ignore the setting (list-path callers: dg_scene_mobj_states_at). */
typedef struct dg_state_rec { char sprite[4]; uint8_t frame; uint8_t full_bright; int16_t tics; int32_t next_state; } dg_state_rec;
typedef struct dg_mobj_info_rec { int32_t doomednum, spawn_state, death_state, xdeath_state; } dg_mobj_info_rec;
#define DG_MOBJ_THINKERS 1u
/* Copies both tables, decodes the sprite frames of the live chains (new ids are appended, none moves) and drops the event list.
 * Takes effect at the next dg_upload_scene; dg_build_lists and dg_scene_mobj_states_at see it at once.  flags 0 turns the setting off
 * and drops the tables (the table arguments are not read).  DG_ERR_INVALID: a NULL scene or table, unknown bits, n_states outside
 * [1, 65536], n_infos < 0, tics < -1 (the reference's i16 count would wrap below -1: out of contract), a next_state or an info state
 * outside [0, n_states).  DG_ERR_WAD: a sprite lump of a live chain does not decode. */
int dg_scene_set_mobj_thinkers(dg_scene *s, uint32_t flags, const dg_state_rec *states, int n_states,
                               const dg_mobj_info_rec *infos, int n_infos);
/* The reference's everything-keys at tics E = (timestamp * 35.0f) as u32, after the E-th mutate and before the next:
 *   DG_MOBJ_KILL     to the type's death_state unless that is 0
 *   DG_MOBJ_EXPLODE  to its xdeath_state unless that is 0, else as DG_MOBJ_KILL
 *   DG_MOBJ_RESPAWN  to its spawn_state
 * An event whose target chain is not live does not move that object.  The events are part of the setting: a list of at most 16 per
 * scene, in non-decreasing tics (of equal tics the later call acts last), which a ctx takes at dg_upload_scene.  what = 0 clears the list.
 * DG_ERR_INVALID: a NULL scene, the setting off, another `what`, tics below the last event's, a 17th event. */
#define DG_MOBJ_KILL 1
#define DG_MOBJ_EXPLODE 2
#define DG_MOBJ_RESPAWN 3
int dg_scene_mobj_event(dg_scene *s, int what, float timestamp);
/* Every map object's state at `timestamp` as this library draws it with no view state (out[i].mobj = i): the thinker's state for an
 * object it drives, else the scene's.  n must equal dg_scene_mobj_count. */
int dg_scene_mobj_states_at(const dg_scene *s, float timestamp, dg_mobj_state *out, int n);

/* ---- context ------------------------------------------------------------------------------------------------ */
typedef struct dg_config {
    int32_t device;        /* HIP device ordinal */
    int32_t width, height; /* frame size (the reference's SCREEN_WIDTH/HEIGHT, src/game.rs:28-29); any width (a multiple of 4 takes the faster read-out) */
    int32_t max_batch;     /* frames per submission */
    int32_t slots;         /* in-flight submissions (>= 1); each owns a framebuffer slab of max_batch frames */
    int32_t host_threads;  /* list-generation threads for dg_render_views / dg_submit_views (0 = the process's CPU share: affinity mask and cgroup CPU quota, capped at 16).
                            * The default assumes ONE ctx per container quota: a process tree with several contexts (one rank per GPU) passes each its
                            * part of the quota, as bench.py does (default_host_threads) */
    int32_t front_end;     /* DG_FE_*: where the per-column half of Segs::process_sidedef / draw_map_objects runs */
} dg_config;

/* dg_config.front_end: how much of the front end (mod.rs:61-104, segs.rs:121-590, sidedef_visplanes.rs, map_objects.rs) runs on the GPU.
 *   DG_FE_HOST         everything on the host: it walks every screen column and ships finished span lists (what dg_draw_lists consumes)
 *   DG_FE_DEVICE       the host does the per-seg half (BSP order, transform, clip, projection: segs.rs:353-590,121-200) and ships per-seg /
 *                      per-sprite records; one GPU lane per screen column does segs.rs:202-345, sidedef_visplanes.rs and
 *                      map_objects.rs:130-209.  A frame that exceeds a device-side capacity is redone through DG_FE_HOST transparently
 *                      (same pixels either way).
 *   DG_FE_DEVICE_SEGS  the per-seg half runs on the GPU too (one lane per seg / map object, one wavefront per frame for what depends on
 *                      the BSP order): the host ships 88 bytes per view and nothing else (with per-view game state,
 *                      dg_submit_views_state: plus one copy of the sector lights and map-object states per view; with per-view poses,
 *                      dg_submit_views_poses: plus 20 bytes per moved object; with per-view surfaces, dg_submit_views_surfaces: plus
 *                      24 bytes per sidedef entry and 16 bytes per sector entry).  Frames it cannot
 *                      judge (a reference panic, a per-frame capacity: 256 parts after culling, 512 map objects in view, 2 560 columns)
 *                      and maps in which a texture / flat lookup would panic fall back to DG_FE_DEVICE / DG_FE_HOST transparently.
 *                      Costs device memory per ctx: max_batch x segs x 41 B of candidate rows + occupancy bits, plus max_batch x segs x 21 B for maps with
 *                      more than 307 segs (candidate lists longer than shared memory holds); when that allocation fails the ctx simply
 *                      keeps the host's per-seg half (DG_FE_DEVICE).
 *   DG_FE_AUTO         DG_FE_DEVICE or DG_FE_DEVICE_SEGS per batch, whichever is the faster way for it: the GPU takes the per-seg half when
 *                      nothing is in flight (the host's time would be exposed), until a seg-walk batch has been timed, or when the host has been measured to be the slower
 *                      side (few host threads, small frames); batches of fewer than 64 views always use the host walker.  The pixels
 *                      are the same whichever is picked; dg_timing.front_end says which one it was.  The choice rests on wall-clock
 *                      measurements (host time per view, kernel time of finished batches): which front end — and therefore which
 *                      instruction stream, and which fallback counters — a given batch gets is NOT reproducible from run to run.
 *                      Ask for DG_FE_DEVICE or DG_FE_DEVICE_SEGS where that matters. */
enum { DG_FE_AUTO = 0, DG_FE_HOST = 1, DG_FE_DEVICE = 2, DG_FE_DEVICE_SEGS = 3 };
/* dg_timing.front_end of a 2-D map submission (dg_submit_map_views); never a dg_config.front_end. */
enum { DG_FE_MAP = 4 };

int dg_create(const dg_config *cfg, dg_ctx **out);
void dg_destroy(dg_ctx *ctx);
/* Number of host threads the ctx uses for list generation (after the default / cap has been applied). */
int dg_ctx_host_threads(const dg_ctx *ctx);
/* Submissions in which a device-side capacity was exceeded: the column scratch of the device column walk (the frames concerned
 * are redone through the host list path, see dg_ctx_redone_frames).  Same pixels either way; a workload that keeps hitting it
 * should raise DOOMGPU_FE_COLUMN_SLOTS.
 * Error reporting differs from the reference in one documented way: BSP subtrees that cannot contribute to the frame are not
 * walked, so a panic the reference would raise while processing a seg in such a subtree
 * (segs.rs:140-145,431-436) is not reported as DG_ERR_RENDER; missing texture / flat lookups disable the skipping for the map. */
int dg_ctx_fallbacks(const dg_ctx *ctx, uint64_t *front_end);
/* Frames that were redone one at a time through the host list path because THEY overflowed a capacity of the device column walk
 * (the other frames of their batch were kept); a frame that does not fit the single-frame scratch either makes the whole batch go
 * through DG_FE_HOST, which dg_ctx_fallbacks counts like every overflow event. */
int dg_ctx_redone_frames(const dg_ctx *ctx, uint64_t *frames);
/* Copy palette, texel planes, flats to HBM (immutable per map). The scene must outlive the ctx's use of it. */
int dg_upload_scene(dg_ctx *ctx, const dg_scene *scene);

/* ---- full path ---------------------------------------------------------------------------------------------- */
/* Synchronous: render n views; if rgb24_out != NULL copy n*3*W*H bytes to host memory.  Uses slot 0. */
int dg_render_views(dg_ctx *ctx, const dg_view *views, int n, uint8_t *rgb24_out);
/* Asynchronous: build lists on the host (blocking), then enqueue the H2D copy on the slot's stream and the kernels behind it on the
 * ctx's kernel stream (all slots' kernels run there, in submission order). */
int dg_submit_views(dg_ctx *ctx, int slot, const dg_view *views, int n);
/* The same with a game-state snapshot per view (states[i] for views[i]; states == NULL: none). */
int dg_submit_views_state(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, int n);
int dg_render_views_state(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, int n, uint8_t *rgb24_out);
int dg_wait(dg_ctx *ctx, int slot);
/* Device address of the slot's framebuffer slab (frame i at + i*3*W*H). Valid until the slot is re-submitted. */
int dg_slot_framebuffer(dg_ctx *ctx, int slot, void **device_ptr);
/* Page-locked host memory for dg_readback / dg_render_views targets (a pageable buffer works too, at a lower PCIe rate). */
void *dg_alloc_host(size_t bytes);
void dg_free_host(void *p);
/* D2H copy of frames [first, first+count) of a completed slot. */
int dg_readback(dg_ctx *ctx, int slot, int first, int count, uint8_t *rgb24_out);
/* The same without waiting: the copy is queued behind the slot's kernels on the slot's own copy stream, so it overlaps the
 * kernels of the NEXT submission on another slot (the reference's caller consumes `pixels.pixels` on the host every frame,
 * src/game.rs:521-525).  rgb24_out should be page-locked (dg_alloc_host) and is complete after dg_wait(slot); every call that renders
 * into the slot again (dg_submit_views*, dg_render_views*, dg_prepare_views, dg_replay_slot, dg_draw_lists) and dg_upload_scene
 * complete it first, so the copy never sees a half-overwritten frame.  One readback in flight per slot. */
int dg_readback_async(dg_ctx *ctx, int slot, int first, int count, uint8_t *rgb24_out);
/* Frame sink without the PCIe copy: one 64-bit checksum per frame of a finished slot, computed on the GPU over the frame's
 * RGB24 bytes taken as little-endian dwords d[0 .. ceil(3*W*H/4)) (a last partial dword is zero-extended):
 *     sum over i of  m ^ (m >> 32),   m = (d[i] ^ (i * 0x9E3779B97F4A7C15)) * 0xBF58476D1CE4E5B9    (all mod 2^64)
 * so a host that holds reference frames (e.g. `pixels.pixels` dumps of the reference, src/game.rs:521-525) can compare
 * thousands of large frames by 8 bytes each.  Waits for the slot like dg_readback. */
int dg_frame_checksums(dg_ctx *ctx, int slot, int first, int count, uint64_t *out);

/* ---- reduced-size frames ------------------------------------------------------------------------------------ */
/* Frame sink for small pictures (thumbnails, a contact sheet, observation tensors): a box downscale on the GPU, so that 1/(fx*fy)
 * of the bytes cross PCIe (a third of that as gray).  Exact, integer only:
 *   oW = ceil(W / fx), oH = ceil(H / fy); output pixel (ox, oy) covers source columns [ox*fx, min(W, ox*fx + fx)) and rows likewise, so a
 *   box at the right or bottom edge covers only the n pixels that exist;
 *   per channel, s = the sum of the box's bytes and  out = floor((2*s + n) / (2*n))  (round to nearest, halves up);
 *   DG_REDUCE_GRAY8 = (77*r + 150*g + 29*b + 128) >> 8  of those three rounded bytes.
 * Output: frame-major, rows top down, tightly packed — 3*oW*oH bytes per frame (r, g, b as in the source) or oW*oH.  fx = fy = 1
 * with DG_REDUCE_RGB24 is a copy. */
enum { DG_REDUCE_RGB24 = 0, DG_REDUCE_GRAY8 = 1 };
typedef struct dg_reduce_desc {
    uint32_t fx, fy;             /* box size in source pixels, each 1..16 */
    uint32_t format;             /* DG_REDUCE_RGB24 or DG_REDUCE_GRAY8 */
    uint32_t reserved;           /* must be 0 */
} dg_reduce_desc;
/* Size of a width x height frame reduced by desc: *out_w, *out_h and the bytes of one reduced frame (each pointer may be NULL).
 * Needs no ctx and no GPU.  DG_ERR_INVALID: a NULL desc, width or height < 1, a factor outside 1..16, an unknown format, reserved != 0. */
int dg_reduced_size(int width, int height, const dg_reduce_desc *desc, int *out_w, int *out_h, size_t *bytes_per_frame);
/* The same arithmetic on the CPU: n_frames RGB24 frames of width x height at src_rgb24 (host memory) into dst (n_frames reduced
 * frames).  For callers without a GPU, and what the GPU paths below are tested against.  DG_ERR_INVALID as dg_reduced_size, and for a
 * NULL src_rgb24 / dst or n_frames < 0. */
int dg_reduce_host(const uint8_t *src_rgb24, int width, int height, int n_frames, const dg_reduce_desc *desc, uint8_t *dst);
/* dg_readback with the downscale in front of the copy: frames [first, first+count) of the slot are reduced on the GPU into a scratch
 * buffer of the slot (allocated by the slot's first reduced readback, grown when a later one needs more) and count reduced frames are
 * copied to dst_host.  Waits for the slot like dg_readback.  DG_ERR_INVALID: a NULL argument, a bad descriptor, a bad frame range. */
int dg_readback_reduced(dg_ctx *ctx, int slot, int first, int count, const dg_reduce_desc *desc, uint8_t *dst_host);
/* The same without waiting, as dg_readback_async: the kernel and the copy are queued behind the slot's kernels on the slot's copy
 * stream.  dst_host should be page-locked and is complete after dg_wait(slot); whatever completes a dg_readback_async first completes
 * this one too.  One readback in flight per slot, plain or reduced: a second one is DG_ERR_INVALID. */
int dg_readback_reduced_async(dg_ctx *ctx, int slot, int first, int count, const dg_reduce_desc *desc, uint8_t *dst_host);
/* Device to device, synchronous, on a stream of the ctx that belongs to no slot: n_frames RGB24 frames of width x height at src_device
 * into dst_device, both on the ctx's device — dg_slot_framebuffer of a finished slot, a tensor's data pointer — and at any alignment.
 * Touches no slot: the route to tensors without a host round trip.  DG_ERR_INVALID: a NULL argument, a bad descriptor, width or
 * height outside [1, 16384], n_frames < 0. */
int dg_reduce_device(dg_ctx *ctx, const void *src_device, int width, int height, int n_frames, const dg_reduce_desc *desc, void *dst_device);
/* GPU time of the last dg_reduce_device call's kernel in milliseconds, from events attached to the dispatch itself (the call's
 * launch and wait are not in it).  DG_ERR_INVALID: a NULL argument, no dg_reduce_device call that launched yet. */
int dg_ctx_reduce_kernel_ms(dg_ctx *ctx, float *ms);

/* Pre-built list path used by benchmarks that want the raster kernels alone: build + upload lists for n views
 * into the slot (untimed), then dg_replay_slot re-runs only the device work (setup + raster kernels). */
int dg_prepare_views(dg_ctx *ctx, int slot, const dg_view *views, int n);
int dg_replay_slot(dg_ctx *ctx, int slot);

/* ---- list path ---------------------------------------------------------------------------------------------- */
/* BitmapColumn, src/renderer/bitmap_render.rs:19-25 (all five values originate as i16: segs.rs:205-220,260) */
typedef struct dg_bitmap_column {
    int16_t x, clipped_top_y, clipped_bottom_y, bottom_y, top_y;
} dg_bitmap_column;

/* BitmapRender, src/renderer/bitmap_render.rs:29-45, restricted to what render_vertical_bitmap_line reads */
typedef struct dg_bitmap_render {
    int32_t bitmap;              /* dg_scene bitmap id (dg_scene_texture_id / dg_scene_sprite_bitmap_id) */
    int16_t light_level;
    int16_t offset_x, offset_y;
    int16_t reserved;
    float line_start_x, line_start_y, line_end_x, line_end_y; /* clipped_line.line */
    float start_offset;                                        /* clipped_line.start_offset */
    int32_t start_x, end_x;
    float bottom_height, top_height;
    uint32_t first_column, n_columns; /* range in the columns array */
} dg_bitmap_render;

/* Visplane, src/renderer/visplanes.rs:17-26; top/bottom stored only for [left, right] */
typedef struct dg_visplane {
    int32_t flat;        /* dg_scene flat id (dg_scene_flat_id); negative = sky (flat name contains "SKY") */
    int16_t height, light_level, left, right;
    uint32_t first_entry; /* index of (top[left], bottom[left]) in the plane_tb array; entries are (top, bottom) pairs */
} dg_visplane;

/* One draw call of the reference, in the order Renderer::render issues them. */
typedef struct dg_draw_cmd {
    uint32_t kind;  /* 0 = replay a dg_bitmap_render (all its columns), 1 = draw_visplane */
    uint32_t index;
} dg_draw_cmd;

typedef struct dg_frame_lists {
    dg_view view;
    const dg_bitmap_render *renders; uint32_t n_renders;
    const dg_bitmap_column *columns; uint32_t n_columns;
    const dg_visplane *visplanes;    uint32_t n_visplanes;
    const int16_t *plane_tb;         uint32_t n_plane_tb; /* int16 count (2 per entry) */
    const dg_draw_cmd *order;        uint32_t n_order;
} dg_frame_lists;

int dg_scene_texture_id(const dg_scene *s, const char *name);                 /* Textures::get (textures.rs:154-179); <0 unknown */
int dg_scene_flat_id(const dg_scene *s, const char *name, float timestamp);   /* Flats::get_animated (flats.rs:103-111); sky => negative */
int dg_scene_sprite_bitmap_id(const dg_scene *s, const char *sprite, uint8_t frame, uint8_t rotation); /* Sprites::get_picture */
int dg_scene_bitmap_size(const dg_scene *s, int bitmap, int *w, int *h);

/* Rasterise caller-built lists for n frames into the slot (synchronous, like dg_render_views). */
int dg_draw_lists(dg_ctx *ctx, int slot, const dg_frame_lists *frames, int n, uint8_t *rgb24_out);

/* The library's own list builder, exposed so a host can inspect / compare lists (and so tests can check the
 * host logic without a GPU).  The returned pointers live in an internal per-thread arena and stay valid
 * until the next dg_build_lists call on the same thread. */
int dg_build_lists(const dg_scene *s, int width, int height, const dg_view *view, dg_frame_lists *out);

/* ---- depth and surface-kind frames --------------------------------------------------------------------------------------- */
/* The third picture of a view next to the screen and the 2-D map: per pixel, the `distance: i16` the reference hands to diminish_color
 * for the draw call that wrote the pixel last (bitmap_render.rs:190-208), and which kind of draw call that was.  Both planes are exact —
 * the reference's own arithmetic, no tolerance — and follow every rule of the colour frame: draw order (the later Pixels::set wins),
 * transparent texels write nothing (bitmap_render.rs:265; a sky bitmap with holes likewise) so the pixel keeps its earlier owner, the
 * row clamps, the `bottom - top <= 1` skip of draw_visplane (visplanes.rs:99, not for sky), columns at x >= W dropped.
 *   uint8_t kind[H][W]        DG_KIND_NONE    never written (Pixels::new zero)
 *                             DG_KIND_COLUMN  render_vertical_bitmap_line: inline wall, masked wall, sprite
 *                             DG_KIND_FLAT    draw_visplane
 *                             DG_KIND_SKY     draw_sky (also where the colour frame is black because the reference would index outside the sky bitmap)
 *   int16_t distance[H][W]    DG_KIND_COLUMN: z of bitmap_render.rs:251;  DG_KIND_FLAT: `wx as i16`, wx = GAME_CAMERA_FOCUS_X * wz / vy
 *                             (visplanes.rs:113,126; an IEEE quotient: the vy == 0 row gives 32767, -32768 or 0 by the `as` rules);
 *                             DG_KIND_NONE and DG_KIND_SKY: 32767, so that a caller who ignores `kind` still sees "far".
 * Negative and saturated distances are stored as they are; light levels and full_bright do not enter.
 * Layout in the slot's framebuffer slab (dg_slot_framebuffer; 3*W*H bytes per frame is exactly what the two planes need): for a
 * submission of n frames  int16 distance[n][H][W]  at the slab's base, then  uint8 kind[n][H][W]  at byte offset 2*n*W*H.
 * A depth submission always takes the host list route (what dg_draw_lists consumes), whatever front end the ctx was created with: the
 * device column walk's records carry no z.  Its rate is therefore bounded by host list generation (dg_timing.host_ms). */
enum { DG_KIND_NONE = 0, DG_KIND_COLUMN = 1, DG_KIND_FLAT = 2, DG_KIND_SKY = 3 };
/* dg_timing.front_end of a depth submission; never a dg_config.front_end. */
enum { DG_FE_DEPTH = 5 };
/* Asynchronous, like dg_submit_views_state (states may be NULL): wall effects, light effects, map-object thinkers and per-view snapshots
 * apply exactly as to a colour frame.  On a depth slot dg_wait, dg_slot_timing (front_end = DG_FE_DEPTH, raster_ms = dg_depth_tiles,
 * setup_ms = 0), dg_slot_framebuffer, dg_upload_scene and every new submission work as usual; dg_readback(_async),
 * dg_readback_reduced(_async), dg_frame_checksums and dg_replay_slot return DG_ERR_INVALID (the planes are not RGB24) and leave the planes
 * intact.  Capacity errors are the host list path's (DG_ERR_CAPACITY). */
int dg_submit_depth_views(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, int n);
/* Synchronous, slot 0: n*W*H int16 into distance and n*W*H bytes into kind (host memory); either may be NULL. */
int dg_render_depth_views(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, int n, int16_t *distance, uint8_t *kind);
/* Synchronous twin of dg_draw_lists for caller-built lists. */
int dg_depth_lists(dg_ctx *ctx, int slot, const dg_frame_lists *frames, int n, int16_t *distance, uint8_t *kind);
/* D2H copy of the planes of frames [first, first+count) of a depth slot; either output may be NULL; count = 0 does nothing.  Waits for
 * the slot like dg_readback.  DG_ERR_INVALID: a bad range, a slot whose last submission is not a depth submission. */
int dg_readback_depth(dg_ctx *ctx, int slot, int first, int count, int16_t *distance, uint8_t *kind);
/* The same planes on the CPU for caller-built lists (dg_build_lists output, or hand-made): needs no ctx and no GPU, and is what the GPU
 * path is tested against.  DG_ERR_INVALID: a NULL scene or frames, width or height outside [1, 16384], n < 0, malformed lists;
 * DG_ERR_RENDER / DG_ERR_CAPACITY as dg_draw_lists.  Either output may be NULL. */
int dg_depth_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, int n, int16_t *distance, uint8_t *kind);

/* ---- object-label frames and per-object screen boxes ---------------------------------------------------------------------- */
/* The fourth picture of a view: per pixel, WHICH thing owns it — the map object or the wall seg whose draw call wrote the pixel last —
 * and per map object how many pixels it owns and their bounding box (what ViZDoom's users know as the labels buffer and the labels
 * list).  Exact, like the depth planes, and under the same rules: draw order (the later Pixels::set wins), transparent texels write
 * nothing so the pixel keeps its earlier owner, the row clamps, the `bottom - top <= 1` skip of draw_visplane, columns at x >= W dropped.
 *   uint8_t  cls[H][W]   DG_LABEL_NONE  no draw call wrote the pixel
 *                        DG_LABEL_WALL  a wall seg's draw call (inline wall or masked middle texture)
 *                        DG_LABEL_MOBJ  a map object's draw call
 *                        DG_LABEL_FLAT  a floor or ceiling (no id: visplanes merge sectors)
 *                        DG_LABEL_SKY   the sky, exactly where the depth frame's kind is DG_KIND_SKY
 *   uint16_t id[H][W]    DG_LABEL_WALL: the seg's index in SEGS;  DG_LABEL_MOBJ: the map object's index (the one dg_scene_set_mobj_state
 *                        and dg_scene_mobj_states_at use);  otherwise 0.
 * An owner tag names the thing a draw record (dg_bitmap_render) belongs to: class << 16 | index, class DG_LABEL_WALL or DG_LABEL_MOBJ.
 * Layout in the slot's framebuffer slab (dg_slot_framebuffer), as for depth: for a submission of n frames  uint16 id[n][H][W]  at the
 * slab's base, then  uint8 cls[n][H][W]  at byte offset 2*n*W*H.
 * boxes[frame][mobj], for every map object of the uploaded scene (dg_scene_mobj_count): `pixels` counts the frame's pixels with class
 * DG_LABEL_MOBJ and that id, x0, y0, x1, y1 is their inclusive bounding box — visible pixels only, occluded and transparent ones are not
 * in it; pixels == 0 gives x0 = y0 = x1 = y1 = -1. */
enum { DG_LABEL_NONE = 0, DG_LABEL_WALL = 1, DG_LABEL_MOBJ = 2, DG_LABEL_FLAT = 3, DG_LABEL_SKY = 4 };
/* dg_timing.front_end of a label submission; never a dg_config.front_end. */
enum { DG_FE_LABELS = 6 };
typedef struct dg_label_box { uint32_t pixels; int16_t x0, y0, x1, y1; } dg_label_box;
/* dg_build_lists with (*owners)[i] set to the owner tag of out->renders[i] (out->n_renders tags; same arena, same lifetime).  The lists
 * are dg_build_lists' byte for byte.  DG_ERR_CAPACITY: the scene has more than 65 536 segs or map objects (an index would not fit). */
int dg_build_lists_owners(const dg_scene *s, int width, int height, const dg_view *view, dg_frame_lists *out, const uint32_t **owners);
/* Asynchronous, like dg_submit_depth_views, and like it always through the host list route whatever front end the ctx has (the device
 * front ends' records carry no owner): wall effects, light effects, map-object thinkers and per-view snapshots apply exactly as to a
 * colour frame.  On a label slot dg_wait, dg_slot_timing (front_end = DG_FE_LABELS, raster_ms = dg_label_tiles + dg_label_boxes,
 * setup_ms = 0), dg_slot_framebuffer, dg_upload_scene and every new submission work as usual; dg_readback(_async),
 * dg_readback_reduced(_async), dg_frame_checksums, dg_replay_slot and dg_readback_depth return DG_ERR_INVALID and leave the planes
 * intact.  The slot's owner array and box table (max_batch x map objects) are device memory of the slot, allocated by its first label
 * submission and again after a dg_upload_scene. */
int dg_submit_label_views(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, int n);
/* Synchronous, slot 0: n*W*H uint16 into id, n*W*H bytes into cls, n * dg_scene_mobj_count boxes into boxes; any may be NULL. */
int dg_render_label_views(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, int n, uint16_t *id, uint8_t *cls, dg_label_box *boxes);
/* Synchronous, for caller-built lists: owners[f] holds frames[f].n_renders owner tags.  DG_ERR_INVALID, before anything is launched: a
 * NULL owners or owners[f] (with n_renders > 0), a tag whose class is not DG_LABEL_WALL or DG_LABEL_MOBJ, a map-object index not below
 * the scene's map-object count, a seg index not below its seg count. */
int dg_label_lists(dg_ctx *ctx, int slot, const dg_frame_lists *frames, const uint32_t *const *owners, int n, uint16_t *id, uint8_t *cls, dg_label_box *boxes);
/* D2H copy of the planes and box rows of frames [first, first+count) of a label slot; any output may be NULL; count = 0 does nothing.
 * Waits for the slot like dg_readback.  DG_ERR_INVALID: a bad range, a slot whose last submission is not a label submission. */
int dg_readback_labels(dg_ctx *ctx, int slot, int first, int count, uint16_t *id, uint8_t *cls, dg_label_box *boxes);
/* GPU time of the two label kernels of the slot's last (label) submission, from the events attached to their dispatches; either may be NULL. */
int dg_slot_label_timing(dg_ctx *ctx, int slot, float *tiles_ms, float *boxes_ms);
/* The same planes and boxes on the CPU: needs no ctx and no GPU, and is what the GPU path is tested against.  Errors as dg_label_lists
 * and dg_depth_lists_host.  Any output may be NULL. */
int dg_label_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, const uint32_t *const *owners, int n,
                        uint16_t *id, uint8_t *cls, dg_label_box *boxes);

/* ---- bundle submissions: colour, depth and labels of the same views from one list build -------------------------------------------- */
/* A caller who wants more than one picture of a view pays host list generation, the upload and a walk over the spans once per picture
 * when each is a submission of its own.  A bundle is ONE submission for any non-empty subset `what` of
 *   DG_BUNDLE_COLOUR  the RGB24 frames of dg_submit_views_state
 *   DG_BUNDLE_DEPTH   the distance and kind planes of a depth submission
 *   DG_BUNDLE_LABELS  the id and class planes and the boxes of a label submission
 * of the same n views: one list build, one upload, the colour kernels of the host list route (only with DG_BUNDLE_COLOUR), and one
 * kernel, dg_bundle_tiles, that walks the spans once for all the other planes and the boxes.  Every part is byte for byte what its own
 * submission gives.
 * Layout in the slot's framebuffer slab (dg_slot_framebuffer), which keeps its size of max_batch * 3*W*H bytes: the requested parts in
 * the order  RGB24 colour 3nWH | int16 distance 2nWH | uint8 kind nWH | uint16 id 2nWH | uint8 cls nWH,  each starting on a 256-byte
 * boundary; dg_bundle_layout gives the byte offsets, a part not in `what` has offset == total.  One submission therefore carries at most
 * dg_bundle_capacity(ctx, what) views: the largest n <= max_batch whose total fits the slab — max_batch for colour alone, about
 * max_batch / 3 for all three parts (it can be 0 for a small max_batch).
 * A bundle always takes the host list route, like depth and label submissions; the box table and the owner array are the slot's lazily
 * allocated ones of the label route.  There is no readback call of its own.  On a slot that holds a bundle:
 *   dg_readback(_async), dg_frame_checksums, dg_readback_reduced(_async)   see the colour frames; DG_ERR_INVALID when `what` has no colour
 *   dg_readback_depth, dg_readback_labels   read the bundle's planes (and boxes); DG_ERR_INVALID when that part was not asked for
 *   dg_replay_slot                          DG_ERR_INVALID (dg_prepare_views is a new submission and replaces the bundle, as on a depth slot)
 *   dg_slot_timing                          front_end = DG_FE_BUNDLE, setup_ms / raster_ms = the colour kernels (0 without colour),
 *                                           total_ms = first kernel's start .. last kernel's end
 *   dg_wait, dg_slot_framebuffer, dg_upload_scene and every new submission work as usual. */
#define DG_FE_BUNDLE 7                      /* dg_timing.front_end of a bundle submission; never a dg_config.front_end */
#define DG_BUNDLE_COLOUR 1u
#define DG_BUNDLE_DEPTH  2u                 /* distance + kind planes   */
#define DG_BUNDLE_LABELS 4u                 /* id + cls planes + boxes  */
typedef struct dg_bundle_offsets { uint64_t colour, distance, kind, id, cls, total; } dg_bundle_offsets;   /* byte offsets in the slot's slab */
/* Pure: no ctx, no GPU.  DG_ERR_INVALID: out == NULL, width or height outside [1, 16384], n <= 0, what == 0 or with unknown bits. */
int dg_bundle_layout(int width, int height, int n, uint32_t what, dg_bundle_offsets *out);
/* The largest n one bundle submission of `what` may carry on this ctx (>= 0); DG_ERR_INVALID: a NULL ctx, a bad `what`. */
int dg_bundle_capacity(const dg_ctx *ctx, uint32_t what);
/* Asynchronous, like dg_submit_views_state (states may be NULL): effects, thinkers and per-view snapshots apply as everywhere.
 * DG_ERR_CAPACITY, before the slot is touched: n outside [1, dg_bundle_capacity(ctx, what)]; with DG_BUNDLE_LABELS also dg_label_lists'
 * scene limit.  DG_ERR_INVALID: a bad `what`, NULL views. */
int dg_submit_bundle_views(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, int n, uint32_t what);
/* The same for caller-built lists; owners (dg_label_lists' owner tags) is needed iff `what` has DG_BUNDLE_LABELS and is not read
 * otherwise.  Refused tags are DG_ERR_INVALID before anything is launched: the slot keeps its earlier content.  Synchronous like
 * dg_draw_lists, up to and including dg_wait: what is left to do is the readback of the parts. */
int dg_bundle_lists(dg_ctx *ctx, int slot, const dg_frame_lists *frames, const uint32_t *const *owners, int n, uint32_t what);
/* The fused per-pixel rule on the CPU: the planes and boxes the bundle's kernel writes, for caller-built lists; needs no ctx and no GPU
 * and is what the kernel is tested against next to dg_depth_lists_host and dg_label_lists_host, which it equals.  Any output may be
 * NULL; owners is needed iff id, cls or boxes is asked for.  Errors as those two calls. */
int dg_bundle_lists_host(const dg_scene *s, int width, int height, const dg_frame_lists *frames, const uint32_t *const *owners, int n,
                         int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes);
/* GPU time of the slot's last (bundle) submission from the events attached to its dispatches: the two colour kernels (0 without
 * DG_BUNDLE_COLOUR) and dg_bundle_tiles (0 for colour alone); any output may be NULL. */
int dg_slot_bundle_timing(dg_ctx *ctx, int slot, float *setup_ms, float *raster_ms, float *tiles_ms);

/* ---- reduced-size depth and label planes ------------------------------------------------------------------------------------------ */
/* The reduced readback of the planes: dg_readback_reduced for distance, kind, id and cls, so that 1/(fx*fy) of their 6 bytes per pixel
 * cross PCIe.  A mean of two object ids, or of a wall and the sky, is meaningless, so no value is computed: every box has ONE
 * representative source pixel and every requested output plane takes that pixel's value unchanged — the distance, kind, id and cls of
 * one output pixel always describe one real source pixel, and the planes stay consistent with each other.
 *   Box geometry is dg_reduce_desc's: oW = ceil(W / fx), oH = ceil(H / fy); box (ox, oy) covers source columns [ox*fx, min(W, ox*fx + fx))
 *   and rows likewise; a box at the right or bottom edge holds only the pixels that exist.
 *   DG_PLANE_POINT    the representative is (min(W-1, ox*fx + fx/2), min(H-1, oy*fy + fy/2)), integer division.
 *   DG_PLANE_NEAREST  the representative is the box pixel with the smallest `distance`, compared as the signed int16 it is stored as;
 *                     ties go to the lowest row, then the lowest column.  Sky and unwritten pixels carry 32767, so any surface in a box
 *                     wins over them; saturated and negative distances take part as stored.  This rule needs a distance plane.
 * fx = fy = 1 is a copy under both rules.  Output: frame-major, rows top down, tightly packed, oW*oH elements per frame and plane.
 * Boxes (dg_label_box) are NOT reduced: they are copied as they are, in full-size pixel coordinates.
 * Out of scope: any pooling other than these two rules, and more than one readback in flight per slot — the colour of a bundle reduced
 * asynchronously plus its planes reduced asynchronously is one asynchronous call and one blocking call. */
enum { DG_PLANE_POINT = 0, DG_PLANE_NEAREST = 1 };
typedef struct dg_plane_reduce_desc {
    uint32_t fx, fy;             /* box size in source pixels, each 1..16 */
    uint32_t rule;               /* DG_PLANE_POINT or DG_PLANE_NEAREST */
    uint32_t reserved;           /* must be 0 */
} dg_plane_reduce_desc;
/* What every call below refuses with DG_ERR_INVALID: a NULL desc, a factor outside 1..16, an unknown rule, reserved != 0, width or height
 * outside [1, 16384], n_frames < 0 or a bad frame range, a source plane without its destination or the reverse, DG_PLANE_NEAREST without
 * a distance plane. */
/* Size of a width x height plane reduced by desc (each pointer may be NULL).  Pure: no ctx, no GPU. */
int dg_plane_reduced_size(int width, int height, const dg_plane_reduce_desc *desc, int *out_w, int *out_h);
/* The rule on the CPU: n_frames planes of width x height (host memory) into their reduced twins.  Needs no ctx and no GPU, and is what
 * the GPU paths below are tested against.  Any source / destination pair may be NULL together. */
int dg_reduce_planes_host(int width, int height, int n_frames, const dg_plane_reduce_desc *desc,
                          const int16_t *distance, const uint8_t *kind, const uint16_t *id, const uint8_t *cls,
                          int16_t *o_distance, uint8_t *o_kind, uint16_t *o_id, uint8_t *o_cls);
/* Device to device, synchronous, on the ctx's stream that belongs to no slot (dg_reduce_device's): the same eight pointers in the ctx's
 * device memory — planes inside dg_slot_framebuffer of a finished slot, tensors' data pointers.  Touches no slot.  The 16-bit planes
 * must be 2-byte aligned (else DG_ERR_INVALID); otherwise any alignment is accepted. */
int dg_reduce_planes_device(dg_ctx *ctx, int width, int height, int n_frames, const dg_plane_reduce_desc *desc,
                            const int16_t *distance, const uint8_t *kind, const uint16_t *id, const uint8_t *cls,
                            int16_t *o_distance, uint8_t *o_kind, uint16_t *o_id, uint8_t *o_cls);
/* GPU time of the last dg_reduce_planes_device call's kernel in milliseconds, from events attached to the dispatch itself.
 * DG_ERR_INVALID: a NULL argument, no dg_reduce_planes_device call that launched yet. */
int dg_ctx_plane_reduce_kernel_ms(dg_ctx *ctx, float *ms);
/* dg_readback_depth / dg_readback_labels with the reduction in front of the copy, on a depth slot, a label slot or a bundle slot:
 * frames [first, first+count) are reduced on the GPU into the slot's scratch buffer (dg_readback_reduced's) and count reduced planes are
 * copied to each output that is not NULL; `boxes` receives count * dg_scene_mobj_count full-size boxes.  distance and kind need a depth
 * part, id, cls and boxes a label part, DG_PLANE_NEAREST a depth part whatever is asked for: DG_ERR_INVALID otherwise, and on a slot that
 * holds neither part (a colour submission, a bundle of colour alone).  All outputs NULL, or count == 0: DG_OK, nothing is done.
 * Waits for the slot like dg_readback, and leaves the slot's planes as they are. */
int dg_readback_planes_reduced(dg_ctx *ctx, int slot, int first, int count, const dg_plane_reduce_desc *desc,
                               int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes);
/* The same without waiting, under every rule of dg_readback_reduced_async: the kernel and the copies are queued behind the slot's
 * kernels on the slot's copy stream; the outputs should be page-locked and are complete after dg_wait(slot); a new submission into the
 * slot and dg_upload_scene complete it first.  One readback in flight per slot, of any kind: a second one is DG_ERR_INVALID. */
int dg_readback_planes_reduced_async(dg_ctx *ctx, int slot, int first, int count, const dg_plane_reduce_desc *desc,
                                     int16_t *distance, uint8_t *kind, uint16_t *id, uint8_t *cls, dg_label_box *boxes);

/* ---- observation tensors ------------------------------------------------------------------------------------------------------------ */
/* The link between the frames and planes the library leaves in device memory and a network on the same GPU: the box downscale of
 * dg_reduce_desc or the representative distance of dg_plane_reduce_desc, a clamp, an affine map and a narrowing, written as uint8,
 * float16, bfloat16 or float32 into a strided (N, C, H, W) destination in ONE pass: contiguous NCHW, channels-last, padded rows, a channel
 * slice of a wider tensor (channel 3 of an RGB-D tensor), a frame stride larger than one observation (slot t mod k of a frame stack).
 * Per output element (frame n, channel c, row oy, column ox), in this order:
 *   1. the integer value v.  DG_OBS_RGB: the byte dg_reduce_host gives for that pixel and channel under (fx, fy, DG_REDUCE_RGB24);
 *      DG_OBS_GRAY: the byte it gives under DG_REDUCE_GRAY8; DG_OBS_DISTANCE: the distance dg_reduce_planes_host gives under
 *      (fx, fy, rule), as the signed int16 it is.  Those functions define v.
 *   2. the clamp: v = min(max(v, lo), hi).
 *   3. the conversion.  DG_OBS_U8: the element is v (needs scale == 1.0f, bias == 0.0f, 0 <= lo, hi <= 255).  Otherwise
 *      o = fl32(fl32((float)v * scale) + bias): two IEEE-754 binary32 roundings, never a fused multiply-add; subnormals are kept, overflow
 *      goes to infinity, the sign of zero follows IEEE (0 * -1 + 0 = +0).  DG_OBS_F32 stores o; DG_OBS_F16 stores o rounded to binary16,
 *      round-to-nearest-even, subnormals kept, overflow to infinity; DG_OBS_BF16 stores o rounded to bfloat16, round-to-nearest-even.
 *      With finite scale and bias no NaN can arise.
 *   4. the store: to dst + (n*strides[0] + c*strides[1] + oy*strides[2] + ox*strides[3]) * element_bytes.  Strides are in ELEMENTS: what a
 *      tensor's .stride() says for its (N, C, H, W) view.
 * Strides: every stride is >= 1; over the dimensions whose extent (n_frames, channels, out_h, out_w) is greater than 1, sorted by stride,
 * each stride must be >= the previous stride times the previous extent (and the largest stride times its extent < 2^62): no two
 * elements share an address.  Only the addressed elements are written; gaps are left as they were.
 * DG_ERR_INVALID: a NULL argument, a factor outside 1..16, an unknown source, rule or dtype, a rule other than 0 for a colour source,
 * reserved != 0, lo > hi or a clamp bound outside int16, a non-finite scale or bias, the DG_OBS_U8 conditions not met, width or height
 * outside [1, 16384], n_frames < 0, strides the rule refuses, a DG_OBS_DISTANCE source that is not 2-byte aligned, a dst not aligned to
 * its element size.  n_frames == 0 does nothing.  The source may otherwise sit at any alignment, as for dg_reduce_device.
 * Out of scope: kind, id and cls planes (categorical: dg_reduce_planes_device serves them), an asynchronous form on a caller's stream,
 * a readback form, frame stacking inside a batch (a view over the frame axis costs nothing). */
enum { DG_OBS_RGB = 0, DG_OBS_GRAY = 1, DG_OBS_DISTANCE = 2 };       /* source: 3, 1, 1 channels */
enum { DG_OBS_U8 = 0, DG_OBS_F16 = 1, DG_OBS_BF16 = 2, DG_OBS_F32 = 3 };
typedef struct dg_obs_desc {
    uint32_t fx, fy;      /* box, each 1..16: the geometry of dg_reduce_desc */
    uint32_t source;      /* DG_OBS_RGB / DG_OBS_GRAY: src is RGB24 frames; DG_OBS_DISTANCE: src is int16 distance planes */
    uint32_t rule;        /* DG_OBS_DISTANCE: DG_PLANE_POINT or DG_PLANE_NEAREST; otherwise must be 0 */
    uint32_t dtype;       /* DG_OBS_* */
    int32_t  lo, hi;      /* clamp of the integer value, lo <= hi, both in [-32768, 32767] */
    float    scale, bias; /* finite */
    uint32_t reserved;    /* must be 0 */
} dg_obs_desc;
/* Shape of the observation of a width x height source under desc (each pointer may be NULL).  Pure: no ctx, no GPU. */
int dg_observed_size(int width, int height, const dg_obs_desc *desc, int *channels, int *out_h, int *out_w, int *element_bytes);
/* The rule on the CPU: n_frames sources at src (host memory) into dst.  Needs no ctx and no GPU, and is what the GPU path is tested
 * against, bit for bit. */
int dg_observe_host(const void *src, int width, int height, int n_frames, const dg_obs_desc *desc, void *dst, const int64_t strides[4]);
/* Device to device, synchronous, on the ctx's stream that belongs to no slot (dg_reduce_device's); touches no slot.  Sources:
 * dg_slot_framebuffer of a finished slot (the distance plane at dg_bundle_layout(...).distance) or any device buffer. */
int dg_observe_device(dg_ctx *ctx, const void *src_device, int width, int height, int n_frames, const dg_obs_desc *desc, void *dst_device, const int64_t strides[4]);
/* GPU time of the last dg_observe_device call's kernel in milliseconds, from events attached to the dispatch itself.
 * DG_ERR_INVALID: a NULL argument, no dg_observe_device call that launched yet. */
int dg_ctx_observe_kernel_ms(dg_ctx *ctx, float *ms);

/* ---- 2-D map view (reference: Game::render with viewing_map, src/game.rs:491-499, 229-309) --------------------------------- */
/* What the window holds after render() in map mode, RGB24 like every frame: black; every linedef without DONTDRAW (flags & 128) in
 * LINEDEFS order, yellow (255, 255, 0) when TWOSIDED (flags & 4) else red (255, 0, 0); then the player arrow in yellow: P->E, R->E, L->E.
 * Points go through transform_vertex_to_point_for_map (f32, the reference's operand order, `as i32`) and lines are rasterised as SDL2's
 * RenderDrawLineBresenham with draw_last (DESIGN.md section 8a states the rule).  The view's x, y, angle and trig are read (trig_valid = 0:
 * cosf / sinf of angle); floor_height and timestamp are not.  The two arrow-head angles always take the host's cosf / sinf.
 * Frames under 40 x 40 are DG_ERR_INVALID (the reference's u32 subtraction underflows), and so is a view whose arrow lands beyond +-2^24
 * pixels after the transform (out of contract). */
typedef struct dg_map_line { int32_t x0, y0, x1, y1; uint32_t rgb; /* r | g<<8 | b<<16 */ } dg_map_line;
/* The lines of one map frame in draw order: drawn linedefs, then the 3 arrow lines (view == NULL: linedefs only).
 * Returns the count; out == NULL or cap too small: count only.  Host only, like dg_build_lists. */
int dg_map_lines(const dg_scene *s, int width, int height, const dg_view *view, dg_map_line *out, int cap);
/* Asynchronous, like dg_submit_views: n map frames into the slot's framebuffer slab, so dg_wait, dg_readback(_async),
 * dg_frame_checksums, dg_slot_framebuffer and dg_slot_timing work on it unchanged (front_end = DG_FE_MAP, raster_ms = the per-frame
 * kernels, setup_ms = the linedef layer when this submission built it, else 0).  The layer does not depend on the view: the first map
 * submission after dg_upload_scene builds it (3*W*H bytes of device memory, kept by the ctx), later ones copy it and draw the arrow.
 * dg_replay_slot re-runs the per-frame kernels.  No scene uploaded: DG_ERR_INVALID; n outside [1, max_batch]: DG_ERR_CAPACITY. */
int dg_submit_map_views(dg_ctx *ctx, int slot, const dg_view *views, int n);
/* Synchronous, slot 0: if rgb24_out != NULL copy n*3*W*H bytes to host memory. */
int dg_render_map_views(dg_ctx *ctx, const dg_view *views, int n, uint8_t *rgb24_out);

/* ---- explored-map frames: the linedefs a session has had on screen, from its label planes ------------------ */
/* dg_submit_map_views draws every linedef, always.  An agent's map observation shows only the lines the agent has seen so far (vanilla's
 * ML_MAPPED, ViZDoom's NORMAL automap mode), and "how many lines did this frame reveal" is the standard exploration signal.  Three pieces,
 * all exact and integer only:
 *   the seen set of a frame   L = linedef count, words = ceil(L / 32) = dg_seen_words.  A row is uint32 seen[words]: bit l & 31 of word
 *                             l >> 5 stands for linedef l, the bits at and above L are 0.  Linedef l is seen by a frame when at least one pixel
 *                             of its label planes has cls == DG_LABEL_WALL and id == k for a seg k of that linedef.  Pixels of any other
 *                             class are ignored whatever their id, and so is a wall pixel whose id is not below the seg count.  DONTDRAW
 *                             lines can be seen (they are never drawn).  This is stricter than vanilla's ML_MAPPED, which marks a line
 *                             when its seg is walked: here a wall wholly covered by sprites (or by nearer walls) is not seen.
 *   the accumulation          the frames of a call are count / run_len consecutive runs of run_len frames, each run one session in time order:
 *                               upto[f]  = carry_in[run] | OR of seen[g] for g <= f in the same run     (carry_in == NULL: all zero)
 *                               total[f] = popcount(upto[f])
 *                               fresh[f] = popcount(upto[f] & ~prev), prev = the run's previous upto row, carry_in[run] for its first frame
 *                               carry_out[run] = the run's last upto row
 *                             count % run_len != 0 or run_len < 1: DG_ERR_INVALID.
 *   the explored map frame    what dg_render_map_views gives (black, LINEDEFS order, a later line over an earlier one, DONTDRAW skipped, the
 *                             colours, the arrow, the 40 x 40 minimum, the +-2^24 rule), except that a linedef is drawn only if its bit is
 *                             set in the frame's mask row.  A mask of all ones gives dg_render_map_views' bytes; where the topmost line at
 *                             a pixel is unseen, the pixel shows the topmost seen line that covers it.
 * The masks travel through the host on purpose (64 bytes per frame for a 500-line map): a caller may pass any mask — all ones, a computer-map
 * pickup — and no slot depends on another slot's stream. */
/* dg_timing.front_end of an explored-map submission; never a dg_config.front_end. */
enum { DG_FE_MAP_EXPLORED = 8 };
/* Host only (no ctx, no GPU), and what the GPU paths are tested against. */
/* words of one seen row of the scene (>= 0); DG_ERR_INVALID: a NULL scene. */
int dg_seen_words(const dg_scene *s);
/* seen[n][words] of n label frames id[n][H][W], cls[n][H][W].  DG_ERR_INVALID: a NULL argument, width or height outside [1, 16384], n < 0;
 * DG_ERR_CAPACITY: the scene limit of label frames (65 536 segs or map objects). */
int dg_seen_lines_host(const dg_scene *s, int width, int height, int n, const uint16_t *id, const uint8_t *cls, uint32_t *seen);
/* The accumulation of n rows of `words` words; carry_in / carry_out hold n / run_len rows; any output may be NULL.  DG_ERR_INVALID: words < 1,
 * n < 0, a bad run_len, seen == NULL with n > 0. */
int dg_seen_accumulate_host(int words, int n, int run_len, const uint32_t *carry_in, const uint32_t *seen, uint32_t *upto, uint32_t *total,
                            uint32_t *fresh, uint32_t *carry_out);
/* One explored map frame (3*W*H bytes) by the literal rule: the lines of dg_map_lines whose linedef's bit is set in mask_row, drawn in order
 * (view == NULL: no arrow).  Errors as dg_map_lines; a NULL scene, mask_row or rgb24_out: DG_ERR_INVALID. */
int dg_explored_map_host(const dg_scene *s, int width, int height, const dg_view *view, const uint32_t *mask_row, uint8_t *rgb24_out);
/* Device to device: seen_dev[n][words] of the planes id_dev[n][H][W], cls_dev[n][H][W] — planes inside dg_slot_framebuffer of a finished
 * slot, tensors' data pointers (the planes are the caller's: an id at or beyond the seg count is ignored).  Synchronous, on the ctx's stream
 * that belongs to no slot (dg_reduce_device's); touches no slot.  id_dev must be 2-byte and seen_dev 4-byte aligned (else DG_ERR_INVALID),
 * cls_dev sits anywhere.  Needs an uploaded scene (DG_ERR_INVALID without one); the seg -> linedef table is uploaded by the first call
 * after dg_upload_scene.  Other errors as dg_seen_lines_host. */
int dg_seen_lines_device(dg_ctx *ctx, int width, int height, int n, const uint16_t *id_dev, const uint8_t *cls_dev, uint32_t *seen_dev);
/* The seen rows of frames [first, first + count) of a label slot, or of a bundle slot with a label part, accumulated as above: the slot is
 * made final as by dg_readback_labels, both kernels run over the slot's planes on the no-slot stream (the planes stay as they are), and the
 * small rows are copied back.  All pointers are host pointers: carry_in / carry_out count / run_len rows, upto count rows, total / fresh count
 * entries; any output may be NULL.  The scratch rows (max_batch x words) are the ctx's, allocated at first use.  DG_ERR_INVALID: any other
 * slot content, a bad range, a bad run_len.  count == 0: DG_OK, nothing is done. */
int dg_slot_seen_lines(dg_ctx *ctx, int slot, int first, int count, int run_len, const uint32_t *carry_in, uint32_t *upto, uint32_t *total,
                       uint32_t *fresh, uint32_t *carry_out);
/* GPU time of the last dg_seen_lines_device / dg_slot_seen_lines call's kernels in milliseconds, from events attached to the dispatches:
 * dg_seen_lines, and dg_seen_accumulate + dg_seen_counts (0 after dg_seen_lines_device).  Either output may be NULL.  DG_ERR_INVALID: a NULL
 * ctx, no such call that launched yet. */
int dg_ctx_seen_kernel_ms(dg_ctx *ctx, float *lines_ms, float *accumulate_ms);
/* Asynchronous, exactly like dg_submit_map_views, with mask = host uint32 [n][words] (copied before the call returns): n explored map frames
 * into the slot's framebuffer slab.  It is a colour frame: dg_wait, dg_readback(_async), dg_frame_checksums, dg_readback_reduced(_async),
 * dg_slot_framebuffer work unchanged; dg_slot_timing gives front_end = DG_FE_MAP_EXPLORED, raster_ms = the per-frame kernels (dg_map_explored
 * and the arrow), setup_ms = the cover upload when this submission made one, else 0.  The cover (4*W*H bytes and the chains of the pixels
 * that several lines cover) does not depend on the view or the mask: the first explored submission after dg_upload_scene builds it on the
 * host and uploads it, the ctx keeps it.  dg_replay_slot re-runs the per-frame kernels: the slot keeps the mask rows in device memory
 * (max_batch x words, allocated by its first such submission).  Errors as dg_submit_map_views; a NULL mask: DG_ERR_INVALID; a scene with more
 * than 65 536 linedefs: DG_ERR_CAPACITY. */
int dg_submit_explored_map_views(dg_ctx *ctx, int slot, const dg_view *views, int n, const uint32_t *mask);
/* Synchronous, slot 0: if rgb24_out != NULL copy n*3*W*H bytes to host memory. */
int dg_render_explored_map_views(dg_ctx *ctx, const dg_view *views, int n, const uint32_t *mask, uint8_t *rgb24_out);

/* ---- player-centred map frames: the map around the player at a fixed scale, rasterised per frame ------------ */
/* dg_submit_map_views fits the whole level to the frame.  An agent's map observation is the map centred on the player at a fixed number
 * of pixels per map unit, usually heading up (ViZDoom's am_followplayer + am_rotate + am_scale, the egocentric top-down map): every
 * line's position then depends on the view, and the lines are rasterised per frame.  Everything is exact.
 *   the point of a map vertex (vx, vy)   every operation in f32 in this order, no contraction:
 *                             dx = vx - view.x, dy = vy - view.y
 *                             DG_EGO_ROTATE:  r = dx*sin_a - dy*cos_a,  f = dx*cos_a + dy*sin_a     without it:  r = dx, f = dy
 *                             X = f32_as_i32(floorf((float)(W/2) + r*scale)),  Y = f32_as_i32(floorf((float)(H/2) - f*scale))
 *                             (W/2, H/2: integer divisions; floorf, so that the column and row left of 0 do not fold onto 0).  The player
 *                             sits at pixel (W/2, H/2).  view.floor_height and view.timestamp are not used; trig_valid = 0 is filled as
 *                             everywhere else.
 *   the frame                 black; the linedefs in LINEDEFS order, DONTDRAW (flags & 128) skipped, a later line over an earlier one, yellow
 *                             when TWOSIDED else red (the map view's colours), each from the point of v1 to the point of v2 by the SDL line
 *                             rule of the map view, points outside the frame dropped.  With a mask row (uint32[dg_seen_words], the layout of
 *                             the explored-map frames) a linedef is drawn only if its bit is set; no mask: every line.
 *   the arrow                 DG_EGO_ARROW: the three lines P->E, R->E, L->E last, in yellow.  Their four map-space points are the map view's
 *                             (Vertex::rotate literally, the host's cosf / sinf for the two head angles) with the lengths
 *                             len = ((float)W / 16.0f) / scale and alen = ((float)W / 32.0f) / scale, then through the point rule.  The libm
 *                             caveat of the map view applies to the arrow and to nothing else.
 * In contract, checked on the host per call and per view (anything else: DG_ERR_INVALID, the frame index in the message): W, H in
 * [16, 16384]; scale finite and in [2^-10, 64]; no unknown flag bits; view.x, view.y finite with |x|, |y| <= 65536; cos_a, sin_a finite
 * with |cos_a|, |sin_a| <= 1.  Consequence: WAD vertices are i16, so |r|, |f| <= 2 * 98304 and every transformed coordinate lies within
 * +-2^24 — the line rule's precondition holds for every line of every in-contract view, and no per-line error can arise on the device.
 * A scene with more than 65 535 linedefs: DG_ERR_CAPACITY; one with no linedefs: DG_ERR_INVALID. */
typedef struct dg_ego_map { float scale; uint32_t flags; } dg_ego_map;   /* scale: pixels per map unit */
enum { DG_EGO_ROTATE = 1u,   /* heading up; without it north up, as the reference's map */
       DG_EGO_ARROW  = 2u }; /* the player arrow on top */
/* dg_timing.front_end of a player-centred map submission; never a dg_config.front_end. */
enum { DG_FE_MAP_EGO = 9 };
/* The lines of one frame in draw order: the drawn linedefs, then the arrow's three if the flags ask for them.  Returns the count; sizing
 * and overflow as dg_map_lines (`out` is written only when cap holds them all).  A NULL scene, view or params: DG_ERR_INVALID. */
int dg_ego_map_lines(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, dg_map_line *out, int cap);
/* One frame (3*W*H bytes) by the literal rule: the lines above whose linedef's bit is set in mask_row (NULL: all), drawn in order point by
 * point.  A NULL scene, view, params or rgb24_out: DG_ERR_INVALID. */
int dg_ego_map_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                    uint8_t *rgb24_out);
/* Asynchronous, exactly like dg_submit_map_views: n frames at the ctx's size into the slot's framebuffer slab, one dg_ego_map for the whole
 * submission, mask = NULL (every line) or host uint32 [n][dg_seen_words] (copied before the call returns).  It is a colour frame: dg_wait,
 * dg_readback(_async), dg_frame_checksums, dg_readback_reduced(_async), dg_slot_framebuffer work unchanged; dg_slot_timing gives
 * front_end = DG_FE_MAP_EGO, raster_ms = the per-frame kernel (dg_ego_tiles), setup_ms = the line-table upload when this submission made
 * one, else 0.  The table (20 bytes per linedef) is uploaded by the first such submission after dg_upload_scene; nothing is allocated at
 * dg_create.  dg_replay_slot re-runs the kernel: the slot keeps the views, the arrow lines and the mask rows in device memory (the mask
 * buffers of the explored-map frames).  These submissions never feed DG_FE_AUTO's measurements or the fallback counters.  Errors as
 * above, and as dg_submit_map_views for the slot, the batch size and the scene. */
int dg_submit_ego_map_views(dg_ctx *ctx, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask);
/* Synchronous, slot 0: if rgb24_out != NULL copy n*3*W*H bytes to host memory. */
int dg_render_ego_map_views(dg_ctx *ctx, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask, uint8_t *rgb24_out);

/* ---- player movement from recorded keys (reference: Game::process_down_keys + update_current_player_height, src/game.rs:314-389) -- */
/* A walk is a play-through as the reference would move it: a start pose, --turbo, and one key mask per 35 Hz tic.  The state after t tics
 * (t = 0: Game::new) is process_down_keys applied t times, literally in f32 (DESIGN.md section 8e states the order and the operands); the
 * turns and moves take the host's cosf / sinf, so the libm caveat of trig_valid = 0 applies.  Bits 6 and 7 of a mask are ignored.
 * floor_height starts at 0.0 and follows get_sector_from_vertex after every move: a position in a sector replaces it (a mid-tic one too),
 * a position in no sector leaves it.  Opt-in: nothing changes for callers who fill dg_view themselves. */
#define DG_KEY_LEFT 1u
#define DG_KEY_RIGHT 2u
#define DG_KEY_UP 4u
#define DG_KEY_DOWN 8u
#define DG_KEY_ALT 16u      /* either Alt */
#define DG_KEY_SHIFT 32u    /* either Shift */
typedef struct dg_walk dg_walk;
typedef struct dg_walk_desc {
    float x, y, angle;          /* OverridePlayer; ignored when from_player_start != 0 (Player1Start) */
    int32_t from_player_start;
    int32_t turbo;              /* percent, the reference's i16 --turbo (default 100); outside i16: DG_ERR_INVALID */
    const uint8_t *keys;        /* keys[t] = keys held during tick t + 1; copied */
    uint32_t n_tics;            /* 0 .. 1 << 22 */
} dg_walk_desc;
/* The poses of all tics are worked out here (host, serial).  The scene must outlive the walk.  DG_ERR_INVALID: a NULL argument, keys == NULL
 * with n_tics > 0, n_tics above 1 << 22, turbo outside i16, from_player_start on a map without a Player1Start.  A walk is not thread-safe. */
int  dg_walk_create(const dg_scene *s, const dg_walk_desc *d, dg_walk **out);
void dg_walk_free(dg_walk *w);
int  dg_walk_tics(const dg_walk *w);
/* Floor lookups the walk needs: the start position, then one per move that ran (at most four per tic). */
int  dg_walk_probe_count(const dg_walk *w);
/* out[t] = floor_height after t tics; n must be tics + 1.  Locates on the host (one BSP descent per probe) if the walk is not located yet. */
int  dg_walk_floors(dg_walk *w, float *out, int n);
/* out[i] = the view at timestamps[i]: the pose and floor after t = min((timestamp * 35.0f) as u32, tics) tics (NaN and <= 0: 0), the four
 * trig fields as with trig_valid = 0, timestamp = timestamps[i], trig_valid = 1 — an ordinary dg_view array for every submit / render / map
 * call.  Timestamps may come in any order.  Host only; locates on the host if the walk is not located yet. */
int  dg_walk_views(dg_walk *w, const float *timestamps, int n, dg_view *out);
/* The floors of all these walks in one pass on the GPU (one lane per probe, then a device-wide scan); synchronous, and the slots in flight
 * are left alone.  Walks that are located already are skipped; afterwards dg_walk_floors / dg_walk_views on these walks do no BSP descent.
 * DG_ERR_INVALID: a NULL argument, no scene uploaded, a walk created on another scene than the one uploaded.  DG_ERR_CAPACITY: more
 * than 1 << 26 probes in one call.  The first call after dg_upload_scene uploads the scene's node and leaf tables. */
int  dg_ctx_locate_walks(dg_ctx *ctx, dg_walk *const *walks, int n_walks);

/* ---- per-view map-object poses (reference: MapObject.position / .angle, src/map_objects.rs:11-17) ---------- */
/* The reference's draw_map_objects reads every object's position and angle on every frame and asks get_sector_from_vertex for the
 * position's sector on every frame (src/renderer/map_objects.rs:55,74,99-116): a caller who moves a monster, a projectile or another
 * player sees it move.  A dg_view_poses says where the objects of ONE view are, on top of where the THINGS lump put them:
 *   an entry overrides the object's x, y and angle for that view only; every object without an entry stands as loaded;
 *   what follows from the position is derived again by the reference's rule: sector = get_sector_from_vertex(x, y), hence the light
 *     level the object is drawn with (unless full-bright) and its z = sector.floor_height;
 *   an object whose sector is None is not drawn in that view (map_objects.rs:100-104);
 *   of two entries for one object in one view the later wins, as in dg_view_state;
 *   an object index out of range is DG_ERR_INVALID, the frame named in the message;
 *   the floats are taken as given, NaN and infinities included — the BSP descent still ends: a NaN comparison takes the right child
 *     every time;
 *   dg_view_state entries, the map-object thinkers, the light effects and the wall effects compose unchanged; a dg_view_state entry and
 *     a pose entry for the same object are independent (one says what it looks like, the other where it is).
 * The 2-D map submissions take no poses and draw no objects, except the *_things map submissions (section 8u), which draw every object's
 * marker where its pose puts it.  Every front end gives the same pixels; with DG_FE_DEVICE_SEGS (and
 * DG_FE_AUTO when it picks the seg walk) the host ships only the entries, and two kernels in front of the seg walk write the batch's
 * rows [frame][object] and find the moved objects' sectors on the GPU (device memory per slot: max_batch x map objects x 16 B of rows
 * and 20 B of entry staging, taken at dg_upload_scene; when that allocation fails, batches with poses take the host walker — same
 * pixels, counted by dg_ctx_fallbacks). */
typedef struct dg_mobj_pose  { int32_t mobj; float x, y, angle; } dg_mobj_pose;   /* MapObject.position / .angle for ONE view */
typedef struct dg_view_poses { const dg_mobj_pose *poses; uint32_t n; } dg_view_poses;
typedef struct dg_mobj_placed { float x, y, angle; int32_t sector; } dg_mobj_placed; /* sector < 0: get_sector_from_vertex gave None */
/* dg_submit_views_state / dg_render_views_state with poses[i] for views[i].  states may be NULL; poses == NULL behaves exactly as
 * those two calls.  DG_ERR_INVALID also for an entry array that is NULL with n > 0. */
int dg_submit_views_poses(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n);
int dg_render_views_poses(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n, uint8_t *rgb24_out);
/* dg_submit_bundle_views with poses (NULL: exactly that call).  A bundle of one part is the depth or the label submission. */
int dg_submit_bundle_views_poses(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, int n, uint32_t what);
/* dg_build_lists / dg_build_lists_owners for a view with poses (poses may be NULL: none; owners may be NULL: not wanted).  The owner
 * tag of a moved object keeps the object's index.  Feeds dg_draw_lists and the dg_*_lists_host functions; host only. */
int dg_build_lists_poses(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, dg_frame_lists *out, const uint32_t **owners);
/* get_sector_from_vertex for n points on the host: sector_out[i] = the sector index of (x[i], y[i]), or -1 for None.  n = 0 does
 * nothing.  DG_ERR_INVALID: a NULL argument, n < 0. */
int dg_scene_sectors_at(const dg_scene *s, const float *x, const float *y, int n, int32_t *sector_out);
/* Every map object's pose and sector as loaded.  n must equal dg_scene_mobj_count. */
int dg_scene_mobj_poses(const dg_scene *s, dg_mobj_placed *out, int n);
/* The pose rows the frames [first, first + count) of the slot's last submission were drawn with: out[count][dg_scene_mobj_count], read
 * from wherever that submission's front end keeps them — after a seg-walk batch with poses the rows its two kernels wrote in device
 * memory, otherwise the rows the host walker derives from the kept entries.  Waits for the slot like dg_readback; count = 0 does
 * nothing.  DG_ERR_STATE: a slot that holds no view submission (an empty slot, a 2-D map submission, caller-built lists);
 * DG_ERR_INVALID: a NULL out, a bad range. */
int dg_slot_mobj_poses(dg_ctx *ctx, int slot, int first, int count, dg_mobj_placed *out);
/* GPU time of the two pose kernels (dg_mobj_pose_fill, dg_mobj_pose_place) of the slot's last submission, from the events attached
 * to their dispatches; 0 when that submission launched neither (no poses, or not the seg walk). */
int dg_slot_mobj_pose_timing(dg_ctx *ctx, int slot, float *ms);

/* ---- per-view sector heights (reference: Sector.floor_height / .ceiling_height, src/map/sectors.rs) --------- */
/* The reference reads every sector's floor and ceiling height again on every frame (src/renderer/segs.rs:376-402,463-484,
 * src/renderer/map_objects.rs:115): a caller who opens a door, runs a lift or a crusher sees it move.  A dg_view_sectors says what the
 * heights of ONE view are, on top of what the SECTORS lump loaded:
 *   an entry overrides both heights of one sector for that view only; every sector without an entry stands as loaded;
 *   what follows from the heights is derived again by the reference's rule: the portal tests and the upper / lower walls, the
 *     unpegged y offsets (differences of heights), the sky hack's min, the visplane heights, and a map object's z = its sector's floor;
 *   of two entries for one sector in one view the later wins, as in dg_view_poses;
 *   a sector index out of range, or a height outside int16, is DG_ERR_INVALID, the frame named in the message;
 *   ceiling < floor is legal: the reference renders it;
 *   dg_view.floor_height stays the caller's; dg_walk's floors stay the loaded ones;
 *   dg_view_state entries, poses (a moved object stands on its new sector's floor as THIS view has it) and the three effects compose
 *     unchanged.
 * The 2-D map submissions draw no heights and take none.  Every front end gives the same pixels; with DG_FE_DEVICE_SEGS (and DG_FE_AUTO
 * when it picks the seg walk) the host ships only the entries, 12 bytes each, and two kernels in front of the seg walk write the
 * batch's rows [frame][sector] of 4 bytes, which a row-reading variant of the seg-walk kernels then takes the heights from (device
 * memory per slot: max_batch x sectors x 4 B of rows and 12 B of entry staging, taken at dg_upload_scene; when that allocation fails,
 * batches with sector entries take the host walker — same pixels, counted by dg_ctx_fallbacks).  A batch without sector entries
 * launches exactly the kernels it launched before. */
typedef struct dg_sector_heights { int32_t sector; int32_t floor_height; int32_t ceiling_height; } dg_sector_heights;
typedef struct dg_view_sectors   { const dg_sector_heights *heights; uint32_t n; } dg_view_sectors;
/* dg_submit_views_poses / dg_render_views_poses with sectors[i] for views[i].  states and poses may be NULL; sectors == NULL behaves
 * exactly as those two calls.  DG_ERR_INVALID also for an entry array that is NULL with n > 0. */
int dg_submit_views_sectors(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n);
int dg_render_views_sectors(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, uint8_t *rgb24_out);
/* dg_submit_bundle_views_poses with sector heights (NULL: exactly that call).  A bundle of one part is the depth or the label submission. */
int dg_submit_bundle_views_sectors(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, uint32_t what);
/* dg_build_lists_poses for a view with sector heights (poses, sectors and owners may each be NULL).  Feeds dg_draw_lists and the
 * dg_*_lists_host functions; host only. */
int dg_build_lists_sectors(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, const dg_view_sectors *sectors, dg_frame_lists *out, const uint32_t **owners);
/* Every sector's floor and ceiling height as loaded.  n must equal dg_scene_sector_count. */
int dg_scene_sector_heights(const dg_scene *s, int16_t *floor, int16_t *ceiling, int n);
/* The heights the frames [first, first + count) of the slot's last submission were drawn with: out[count][dg_scene_sector_count][2]
 * (floor, ceiling), read from wherever that submission's front end keeps them — after a seg-walk batch with sector entries the rows
 * its two kernels wrote in device memory, otherwise the rows the host walker derives from the kept entries.  Waits and fails like
 * dg_slot_mobj_poses. */
int dg_slot_sector_heights(dg_ctx *ctx, int slot, int first, int count, int16_t *out);
/* GPU time of the row kernels (dg_sector_row_fill, dg_sector_row_scatter) of the slot's last submission, from the events attached to
 * their dispatches; 0 when that submission launched neither (no sector entries, or not the seg walk). */
int dg_slot_sector_height_timing(dg_ctx *ctx, int slot, float *ms);

/* ---- per-view surfaces (reference: SideDef textures and offsets, Sector floor_texture / ceiling_texture) ------ */
/* The reference reads a sidedef's three texture names and two offsets, and a sector's two flat names, again on every frame
 * (src/renderer/segs.rs:121-200,450-469,493-588): a caller who flips a switch, changes a floor's flat or scrolls a wall sees it.  A
 * dg_view_surfaces says what the surfaces of ONE view are, on top of what the SIDEDEFS and SECTORS lumps loaded:
 *   a dg_side_surface overrides all five fields of one sidedef, a dg_sector_flats both flats of one sector, for that view only (a caller
 *     who changes one field copies the others from dg_scene_sidedef_surfaces / dg_scene_sector_flats);
 *   textures are bitmap ids from dg_scene_use_texture (DG_TEX_NONE: "-"), flats are handles from dg_scene_use_flat;
 *   what follows is derived again by the reference's rule: the texture's own width and height in the mapper, holes where a masked
 *     middle appears or disappears, the sky flag of the ceiling flat (the sky hack switches on and off), a floor that becomes sky, an
 *     animated flat by timestamp (by the name's list, as Flats::get_animated, not by the name's position in it);
 *   with dg_scene_set_wall_effects, an overriding texture that is a member of a live animation list animates, and the special-48
 *     scroll is added to the overriding x_offset;
 *   of two entries for one sidedef or one sector in one view the later wins;
 *   an index out of range, a texture id that is neither DG_TEX_NONE nor a wall-texture id of this scene, a flat handle not of this
 *     scene, an offset outside int16, or a NULL array with n > 0 is DG_ERR_INVALID, the frame named in the message;
 *   states, poses, sector heights and the three effects compose unchanged.
 * The 2-D map submissions take none.  Every front end gives the same pixels; with DG_FE_DEVICE_SEGS (and DG_FE_AUTO when it picks the
 * seg walk) the host ships only entries: 16 bytes per sector entry, from which two kernels write the batch's rows [frame][sector] of
 * 8 bytes, and 24 bytes per sidedef entry, sorted per frame, which the seg walk searches by a seg's front sidedef (per slot, taken at
 * dg_upload_scene: device memory max_batch x sectors x 24 B of rows and entries and 64 x max_batch x 24 B of sidedef entries, pinned
 * memory max_batch x sectors x 16 B and the same sidedef table; it does not grow with the sidedef count; when that allocation fails, or a batch holds more than 64 x max_batch sidedef entries, the batch takes the host walker — same pixels,
 * counted by dg_ctx_fallbacks).  A batch without surfaces launches exactly the kernels it launched before. */
#define DG_TEX_NONE (-1)                      /* "-" */
typedef struct dg_side_surface { int32_t sidedef; int32_t tex_mid, tex_low, tex_up; int32_t x_offset, y_offset; } dg_side_surface;
typedef struct dg_sector_flats { int32_t sector; int32_t floor_flat, ceil_flat; } dg_sector_flats;
typedef struct dg_view_surfaces { const dg_side_surface *sides; uint32_t n_sides; const dg_sector_flats *flats; uint32_t n_flats; } dg_view_surfaces;
/* The bitmap id of Textures::get(name), by the loader's case rules: the texture is decoded and appended if the map did not use it (no
 * id moves); "-" gives DG_TEX_NONE (the value of DG_ERR_INVALID, which a NULL argument gives: "-" is the only name that returns it);
 * an unknown name is DG_ERR_WAD.  Call before dg_upload_scene, like dg_scene_sprite_frame: a context refuses batches of a scene that
 * has decoded bitmaps or loaded flats since its upload. */
int dg_scene_use_texture(dg_scene *s, const char *name);
/* A flat handle for the name (>= 0): its lump is loaded if the map did not use it; the name of a member of an animated-flat list stands
 * for that list, and every member is loaded.  A missing lump is DG_ERR_WAD.  Call before dg_upload_scene. */
int dg_scene_use_flat(dg_scene *s, const char *name);
/* The surfaces as loaded: one entry per sidedef / per sector, in index order.  n must equal dg_scene_sidedef_count /
 * dg_scene_sector_count.  (A sidedef whose texture name is unknown to the WAD reports -2 there, and a sector whose flat lump is missing a
 * handle with bit 28 set: neither is valid to submit — the reference panics when it draws them — so an entry for such a sidedef or
 * sector has to name something else in that field.) */
int dg_scene_sidedef_count(const dg_scene *s);
int dg_scene_sidedef_surfaces(const dg_scene *s, dg_side_surface *out, int n);
int dg_scene_sector_flats(const dg_scene *s, dg_sector_flats *out, int n);
/* The _sectors calls with surfaces[i] for views[i]; surfaces == NULL is exactly the _sectors call. */
int dg_submit_views_surfaces(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, const dg_view_surfaces *surfaces, int n);
int dg_render_views_surfaces(dg_ctx *ctx, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, const dg_view_surfaces *surfaces, int n, uint8_t *rgb24_out);
int dg_submit_bundle_views_surfaces(dg_ctx *ctx, int slot, const dg_view *views, const dg_view_state *states, const dg_view_poses *poses, const dg_view_sectors *sectors, const dg_view_surfaces *surfaces, int n, uint32_t what);
int dg_build_lists_surfaces(const dg_scene *s, int width, int height, const dg_view *view, const dg_view_poses *poses, const dg_view_sectors *sectors, const dg_view_surfaces *surfaces, dg_frame_lists *out, const uint32_t **owners);
/* The flat handles the frames [first, first + count) of the slot's last submission were drawn with: out[count][dg_scene_sector_count][2]
 * (floor, ceiling) — after a seg-walk batch with surfaces the rows its two kernels wrote in device memory, otherwise the rows the host
 * walker derives from the kept entries.  Waits and fails like dg_slot_sector_heights. */
int dg_slot_sector_flats(dg_ctx *ctx, int slot, int first, int count, int32_t *out);
/* GPU time of the row kernels (dg_flat_row_fill, dg_flat_row_scatter) of the slot's last submission, from the events attached to their
 * dispatches; 0 when that submission launched neither (no surfaces, or not the seg walk). */
int dg_slot_surface_timing(dg_ctx *ctx, int slot, float *ms);

/* ---- screen pictures: weapon, status bar, crosshair over finished colour frames ----------------------
 * The screen is not the world: a picture is laid over RGB24 frames that are already rendered, in a pass of its own, and is no input of
 * a submission.  The reference has the parts — Pictures::get (src/graphics/pictures.rs:38-47), Bitmap::test_flat_draw
 * (src/graphics/bitmap.rs:28-53), Picture::mirror (pictures.rs:129-147), the weapon states of src/info.rs — and never calls them from
 * render(); this is test_flat_draw without its debugging background, with a free scale, origin and light.
 *
 * dg_scene_use_picture: the handle (>= 0) of the lump `name` anywhere in the WAD — sprite lumps and patches included — by the loader's
 * case rule (to_ascii_uppercase), decoded by the loader's picture decoder and appended to the scene's bitmaps when new (no id moves;
 * the scene's revision changes when a bitmap was added).  The same name gives the same handle.  NULL: DG_ERR_INVALID.  No such lump, or one
 * that does not decode as a picture (a post that runs past the picture's height is an index panic in the reference): DG_ERR_WAD.
 * Call before dg_upload_scene, like dg_scene_use_texture. */
int dg_scene_use_picture(dg_scene *s, const char *name);
int dg_scene_picture_count(const dg_scene *s);
/* Size and offsets of a picture; any output may be NULL.  DG_ERR_INVALID: a NULL scene, not a handle of the scene. */
int dg_scene_picture_info(const dg_scene *s, int picture, int32_t *w, int32_t *h, int32_t *left, int32_t *top);

#define DG_PIC_OFFSETS 1u   /* origin moves left/up by the picture's offsets times the scale (vanilla's V_DrawPatch) */
#define DG_PIC_MIRROR  2u   /* Picture::mirror, pictures.rs:129-147: texel column w-1-tx */
typedef struct dg_screen_picture { int32_t picture; int32_t x, y; uint16_t scale_x, scale_y; int16_t light_level; uint16_t flags; } dg_screen_picture;
/* A batch of n frames brings items[] and first[n + 1]: first[0] = 0, first[] non-decreasing, frame f owns items[first[f] .. first[f + 1])
 * (possibly none).  The rule, all integers but the shade, for picture P of w x h with offsets l, t:
 *   ox = x - (OFFSETS ? l * scale_x : 0),  oy = y - (OFFSETS ? t * scale_y : 0)
 *   the item covers ox <= px < ox + w * scale_x, oy <= py < oy + h * scale_y, clipped to the frame
 *   its texel there is tx = (px - ox) / scale_x (w - 1 - tx under MIRROR), ty = (py - oy) / scale_y
 *   a None texel leaves the pixel alone; Some(v) sets it to diminish_color(palette[v], light_level, 0) — the palette colour at 255
 *   the items of a frame act in list order, later over earlier.
 * With scale 4, flags 0 and light 255 one item is test_flat_draw.  Checked first, for the whole call, and DG_ERR_INVALID with nothing
 * drawn otherwise: every picture a handle of the scene, scales in 1..16, light_level in 0..255, x and y within +-(1 << 20), no unknown
 * flag bits, first[] well formed, width and height in [1, 16384], n_frames >= 0, no NULL argument.
 *
 * dg_overlay_host draws in place on frames[n_frames][height][width][3] in host memory; needs no GPU. */
int dg_overlay_host(const dg_scene *s, uint8_t *frames, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first);
/* The same on frames in device memory on the ctx's device — the caller's, or dg_slot_framebuffer of a finished slot — of any size in
 * [1, 16384]^2, independent of the ctx's; items and first are host arrays, staged in a scratch of the ctx's that grows as needed.  Runs
 * on the ctx's stream that belongs to no slot (dg_reduce_device's) and returns when done.  Every covered pixel is stored once, with the
 * colour of the topmost item that has a Some texel there; a pixel no item sets is neither read nor written.  Needs an uploaded scene;
 * a picture loaded since dg_upload_scene is DG_ERR_INVALID until the scene is uploaded again.  n_frames = 0, or no items: DG_OK, nothing
 * launched. */
int dg_overlay_device(dg_ctx *ctx, void *frames_device, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first);
/* ... on the colour frames [first_frame, first_frame + count) of the slot's last submission, once that is final (waits like dg_wait;
 * frames that overflowed a capacity are redone first): views, caller-built lists, 2-D map, explored-map and player-centred map frames,
 * and the colour part of a bundle at its place in the bundle's layout.  items / first describe `count` frames.  DG_ERR_INVALID: a depth
 * or label slot, a bundle without DG_BUNDLE_COLOUR, an empty slot, a bad frame range, and — nothing drawn — a slot with a
 * dg_readback_async (or reduced one) pending: that copy was promised the frames as rendered.  Afterwards dg_readback(_async),
 * dg_frame_checksums, dg_readback_reduced(_async), dg_reduce_device and dg_observe_device see the overlaid frames.  A new submission or
 * dg_replay_slot renders over the pictures; calling twice draws twice. */
int dg_slot_overlay(dg_ctx *ctx, int slot, int first_frame, int count, const dg_screen_picture *items, const uint32_t *first);
/* GPU time of the last dg_overlay_device / dg_slot_overlay call's kernel in milliseconds, from events attached to the dispatch itself.
 * DG_ERR_INVALID: a NULL argument, no such call that launched yet. */
int dg_ctx_overlay_kernel_ms(dg_ctx *ctx, float *ms);

/* ---- floor-textured player-centred map frames: the sectors' floors under the lines ---------------------------- */
/* The player-centred map frames above are lines on black.  The map most users of this vocabulary know draws the sectors' floor textures
 * under the lines (ViZDoom's set_automap_render_textures, ZDoom's am_textured).  A floor-map frame of a view takes the same dg_ego_map:
 * DG_EGO_ROTATE, DG_EGO_ARROW and the contract (W, H in [16, 16384], scale in [2^-10, 64], |view.x|, |view.y| <= 65536, |cos_a|,
 * |sin_a| <= 1, at most 65 535 linedefs) mean what they mean there, and a pixel on which dg_ego_map_host draws a line or the arrow has
 * exactly that colour.  Every other pixel (X, Y), every operation in f32 in this order, no contraction, inv = 1.0f / scale once per call:
 *   1. the map point          r = ((float)(X - W/2) + 0.5f) * inv,  f = ((float)(H/2 - Y) - 0.5f) * inv     (the pixel's centre)
 *                             DG_EGO_ROTATE:  dx = r*sin_a + f*cos_a,  dy = f*sin_a - r*cos_a      without it:  dx = r, dy = f
 *                             mx = view.x + dx,  my = view.y + dy
 *   2. the leaf               from the BSP's root, left of or on a node's partition (Vertex::is_left_of_line, cross <= 0) to its left
 *                             child: get_sector_from_vertex (src/renderer/bsp.rs:9-44).  A leaf none of whose segs has a sidedef on its
 *                             side: background.
 *   3. inside the subsector   for every seg v1 -> v2 of the leaf in lump order:
 *                             (mx - v1x) * (v2y - v1y) - (my - v1y) * (v2x - v1x) < 0.0f (strictly behind the seg): background.  The BSP
 *                             gives every point of the plane a leaf, solid rock and the outside of the level included.
 *   4. the floor              its flat: a dg_sector_flats entry of the view for the sector, else the scene's; an animated flat by
 *                             view.timestamp (Flats::get_animated).  A missing flat or a sky floor: background.  Its light: a
 *                             dg_sector_light entry of the view, else the light effect's level at the timestamp with DG_LIGHT_THINKERS, else
 *                             the scene's.  Both are what the colour frame of the same view draws the floor with.
 *   5. texel and shade        tx = f32_as_i32(floorf(mx)) & 63, ty = f32_as_i32(floorf(my)) & 63, the texel flat[ty][tx] (both axes
 *                             positive, src/renderer/visplanes.rs:119-125); the colour diminish_color(palette[texel], light, 0).
 * Background is (0, 0, 0).  |mx|, |my| stay below 2^24 whenever scale >= 2^-9 or W, H <= 8192 (|r|, |f| <= 8192.5 / scale, |dx|, |dy| <=
 * |r| + |f|); the rule is defined beyond that too (the conversion saturates).
 * With a mask row (the layout of dg_submit_ego_map_views) a linedef is drawn only if its bit is set, and a sector is shown only if at
 * least one linedef with a sidedef facing it has its bit set; every other sector's pixels are background.  No mask: every line, every sector.
 * state / surfaces: NULL, or the view's game state and surfaces — only state->lights and surfaces->flats are read (entries validated as
 * for dg_submit_views_surfaces: an index out of range, a handle not of this scene, a NULL array with n > 0 are DG_ERR_INVALID).
 * dg_timing.front_end of such a submission; never a dg_config.front_end. */
enum { DG_FE_MAP_FLOOR = 10 };
/* One frame (3*W*H bytes) by the literal rule, with the scene's light effects as last set.  Everything is checked before the first byte
 * is written.  A NULL scene, view, params or rgb24_out: DG_ERR_INVALID. */
int dg_floor_map_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                      const dg_view_state *state, const dg_view_surfaces *surfaces, uint8_t *rgb24_out);
/* Asynchronous, exactly like dg_submit_ego_map_views: n frames at the ctx's size into the slot's framebuffer slab; states / surfaces NULL
 * or [n].  Every check comes first: a refused call leaves the slot as it was.  It is a colour frame like the other map submissions
 * (readbacks, checksums, reduced readbacks, dg_observe_device, dg_replay_slot, dg_slot_overlay; dg_slot_seen_lines refuses it);
 * dg_slot_timing gives front_end = DG_FE_MAP_FLOOR, raster_ms = the per-frame kernel (dg_floor_map_tiles), setup_ms = the upload of the
 * scene's tables (nodes, leaves, segs, the linedefs' sectors and dg_submit_ego_map_views' line table) when this submission made it, else
 * 0.  The host ships 8 bytes per (frame, sector) — the flat and the shade factor of each sector as the view has them — and with a mask
 * dg_floor_seen_sectors builds the sector rows on the GPU.  Errors as dg_submit_ego_map_views; a scene without subsectors: DG_ERR_INVALID. */
int dg_submit_floor_map_views(dg_ctx *ctx, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                              const dg_view_state *states, const dg_view_surfaces *surfaces);
/* Synchronous, slot 0: if rgb24_out != NULL copy n*3*W*H bytes to host memory. */
int dg_render_floor_map_views(dg_ctx *ctx, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                              const dg_view_state *states, const dg_view_surfaces *surfaces, uint8_t *rgb24_out);

/* ---- map objects on the player-centred and floor-textured map frames ------------------------------------------ */
/* ViZDoom's OBJECTS / OBJECTS_WITH_SIZE automap modes, vanilla's am_cheat markers: every map object as its collision box and a heading
 * line, where a dg_view_poses puts it and in the state a dg_view_state or the map-object thinkers give it.
 *   the marker table          per scene, one entry per map object, from the caller (the library ships none, like the state tables of
 *                             dg_scene_set_mobj_thinkers): radius in map units, colour, and which parts are drawn.  flags 0: the object
 *                             has no marker.
 *   which objects are shown   for a view, object i is shown when its marker has a flag set; its sprite_frame for that view is not -1
 *                             (composed as for the colour frame: a dg_view_state entry wins, else the thinker's state at view.timestamp
 *                             with DG_MOBJ_THINKERS, else the scene's); and its position is finite with |x|, |y| <= 32768 (the view's
 *                             later dg_view_poses entry for i, else as loaded).  An object that fails one of these is not drawn in that
 *                             view; that is no error.  The object's sector plays no part: an object outside every subsector is on the map.
 *   the marker                R = (float)radius, a = the object's angle (the pose entry's, else as loaded), every operation in f32, no
 *                             contraction.  DG_MARK_BOX: c0 = (x-R, y-R), c1 = (x+R, y-R), c2 = (x+R, y+R), c3 = (x-R, y+R) and the
 *                             lines c0->c1, c1->c2, c2->c3, c3->c0 — Doom's own map-axis-aligned collision box, so it turns with the map
 *                             under DG_EGO_ROTATE.  DG_MARK_HEADING: after the box, the line (x, y) -> (x + R*ca, y + R*sa) with
 *                             ca = cosf(a), sa = sinf(a) from the host's libm (the libm caveat of the arrow applies to this line and to
 *                             nothing else; an angle that is not finite has no heading line).  Every endpoint goes through the point rule
 *                             of the player-centred frames unchanged, every line through the SDL line rule of the map view, points outside
 *                             the frame dropped.
 *   draw order and colour     the linedefs as in dg_ego_map_host (with their mask; the mask row does not touch markers), then the objects
 *                             in index order (box lines, then heading), then the arrow; a later line goes over an earlier one.  A marker
 *                             pixel has the marker's rgb, on a floor-textured frame too (rgb 0 is a black pixel, not a floor pixel).
 * In contract: |x|, |y| <= 32768 and R <= 1024 put an endpoint within +-33792, so with |view.x|, |view.y| <= 65536 |r|, |f| <= 2 * 99328,
 * times 64 plus 8192 stays below 2^24 — the line rule's precondition holds for every marker line of every in-contract view. */
typedef struct dg_map_marker { int32_t radius; uint32_t rgb; uint32_t flags; } dg_map_marker;   /* rgb: r | g<<8 | b<<16 */
enum { DG_MARK_BOX = 1u, DG_MARK_HEADING = 2u };   /* flags 0: the object has no marker */
/* Sets the scene's marker table (copied); n must be dg_scene_mobj_count.  markers == NULL && n == 0 drops the table.  DG_ERR_INVALID: a
 * NULL scene, a radius outside [0, 1024], rgb above 0xffffff, unknown flag bits, a wrong n.  The host functions below see the table at
 * once; a ctx takes it at dg_upload_scene, like the other scene settings. */
int dg_scene_set_map_markers(dg_scene *s, const dg_map_marker *markers, int n);
/* The marker lines of one frame in draw order, transformed and unclipped, with the marker's colour.  Returns the count; sizing and overflow
 * as dg_ego_map_lines.  state / poses: NULL, or the view's (entries validated as in dg_submit_views_state / dg_submit_views_poses: an
 * index out of range or a NULL array with n > 0 is DG_ERR_INVALID).  No marker table: 0.  Errors as dg_ego_map_lines; a scene with more
 * than 65 536 map objects: DG_ERR_CAPACITY. */
int dg_map_thing_lines(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const dg_view_state *state,
                       const dg_view_poses *poses, dg_map_line *out, int cap);
/* dg_ego_map_host / dg_floor_map_host with the markers, by the literal rule, with the scene's effects as last set.  With no marker
 * table, or one whose flags are all 0, the bytes are theirs.  Everything is checked before the first byte is written. */
int dg_ego_map_things_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                           const dg_view_state *state, const dg_view_poses *poses, uint8_t *rgb24_out);
int dg_floor_map_things_host(const dg_scene *s, int width, int height, const dg_view *view, const dg_ego_map *params, const uint32_t *mask_row,
                             const dg_view_state *state, const dg_view_surfaces *surfaces, const dg_view_poses *poses, uint8_t *rgb24_out);
/* dg_submit_ego_map_views / dg_submit_floor_map_views with the markers of the table the ctx took at dg_upload_scene; states / poses NULL or
 * [n].  The existing calls and their kernels are untouched: these run dg_ego_thing_tiles / dg_floor_thing_tiles, the same band kernels
 * with one more phase.  Colour frames like every map submission (readbacks, checksums, reduced readbacks, dg_observe_device,
 * dg_slot_overlay, dg_replay_slot); dg_slot_timing gives DG_FE_MAP_EGO / DG_FE_MAP_FLOOR with the new kernel in raster_ms.  Every check
 * comes before the slot is touched.  Per submission the host ships, per frame, a row of shown bits (one per object) and the frame's pose
 * entries after later-wins, sorted by object (20 bytes each); the scene's marker and place tables (28 bytes per object) are uploaded by
 * the first such submission after dg_upload_scene, and the slot keeps what a replay needs in device memory, allocated at first use.  The
 * device never evaluates a trigonometric function.  Errors as the plain calls and as dg_map_thing_lines. */
int dg_submit_ego_map_views_things(dg_ctx *ctx, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                                   const dg_view_state *states, const dg_view_poses *poses);
int dg_render_ego_map_views_things(dg_ctx *ctx, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                                   const dg_view_state *states, const dg_view_poses *poses, uint8_t *rgb24_out);
int dg_submit_floor_map_views_things(dg_ctx *ctx, int slot, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                                     const dg_view_state *states, const dg_view_surfaces *surfaces, const dg_view_poses *poses);
int dg_render_floor_map_views_things(dg_ctx *ctx, const dg_view *views, int n, const dg_ego_map *params, const uint32_t *mask,
                                     const dg_view_state *states, const dg_view_surfaces *surfaces, const dg_view_poses *poses, uint8_t *rgb24_out);

/* ---- line-of-sight queries (vanilla: P_CheckSight) ---------------------------------------- */
/* Is there a clear line from here to there?  A query is the line from (x0, y0) at height z0 to (x1, y1), whose target spans the heights
 * [z1_lo, z1_hi]; sector heights are those of frame `frame`: the scene's, with that frame's dg_view_sectors entries on top (a door
 * that is shut in one frame blocks there alone).  The rule, stated in full in DESIGN.md section 8v and in csrc/sight_core.h:
 *   the line visits the BSP leaves on its way (at a node: the child on the start's side always, the other one unless the end lies
 *   strictly on the start's side); every linedef of a visited leaf that the line crosses (the signs of the four cross products)
 *   blocks it when it is one-sided or its opening is closed (max of the floors >= min of the ceilings), and otherwise narrows the
 *   slope range [lo, hi], which starts as [z1_lo - z0, z1_hi - z0], by its lower and upper edge at the crossing;
 *   visible (1) iff nothing blocked and hi > lo at the end, else 0.
 * IEEE f32 throughout; the result does not depend on the visiting order.  A query with a float that is not finite or beyond 65536 in
 * magnitude is out of contract: 0.  All pointers are host pointers; sectors may be NULL (every frame has the scene's heights), else it
 * holds n_frames elements; n == 0: DG_OK, nothing done.  DG_ERR_INVALID: a NULL required argument, n or n_frames negative, a q[i].frame
 * outside [0, n_frames), a sector entry out of range or a height outside int16 (as dg_submit_views_sectors), a NULL entry array with
 * n > 0.  DG_ERR_CAPACITY: n above 1 << 20. */
typedef struct dg_sight_query { int32_t frame; float x0, y0, z0, x1, y1, z1_lo, z1_hi; } dg_sight_query;
int dg_sight_host(const dg_scene *s, const dg_view_sectors *sectors, int n_frames, const dg_sight_query *q, int n, uint8_t *visible_out);
/* The same on the GPU (dg_sight_queries: one lane per query), bit for bit: on the ctx's stream that belongs to no slot, synchronous,
 * touching no slot.  Needs an uploaded scene (DG_ERR_INVALID without one); its sight tables are uploaded by the first call after
 * dg_upload_scene, the scratch buffers are the ctx's, allocated at first use.  DG_ERR_CAPACITY, before anything is launched: n_frames
 * above max_batch, or a scene whose BSP is deeper than 64 nodes (dg_scene_bsp_depth) — the host call has no such limit. */
int dg_sight_device(dg_ctx *ctx, const dg_view_sectors *sectors, int n_frames, const dg_sight_query *q, int n, uint8_t *visible_out);
/* Which map objects does each of n views see?  One query per (view, map object m): from the view's (x, y) at z0 = view.floor_height +
 * eye_height to the object's (x, y) in that view (its dg_view_poses entry, else as loaded), the target from the floor of the object's
 * sector in that view's heights up to mobj_height[m] above it.  An object whose sector is none, or whose mobj_height is not positive
 * (the caller's way to leave it out), is not visible.  visible_out[n][dg_sight_words]: bit m & 31 of word m >> 5 of row i; the tail
 * bits of a row are 0.  poses and sectors may be NULL, else n elements each.  DG_ERR_INVALID: a NULL required argument, n negative, an
 * entry out of range (as dg_submit_views_sectors), a NULL entry array with n > 0.  The device call (dg_sight_mobjs: one lane per
 * pair, a wavefront per frame and 64 objects) as dg_sight_device, n bounded by max_batch. */
int dg_sight_words(const dg_scene *s);                 /* ceil(map objects / 32); DG_ERR_INVALID: a NULL scene */
int dg_sight_mobjs_host(const dg_scene *s, const dg_view *views, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, float eye_height,
                        const float *mobj_height, uint32_t *visible_out);
int dg_sight_mobjs_device(dg_ctx *ctx, const dg_view *views, const dg_view_poses *poses, const dg_view_sectors *sectors, int n, float eye_height,
                          const float *mobj_height, uint32_t *visible_out);
/* GPU time of the last dg_sight_device / dg_sight_mobjs_device call's kernels in milliseconds, from events attached to the dispatches:
 * the row kernels (dg_sector_row_* and dg_mobj_pose_*; 0 when no frame had entries) and the sight kernel.  Either output may be NULL.
 * DG_ERR_INVALID: a NULL ctx, no such call that launched yet. */
int dg_ctx_sight_kernel_ms(dg_ctx *ctx, float *rows_ms, float *sight_ms);
/* The nodes on the longest way from the BSP's root to a leaf (>= 1); DG_ERR_INVALID: a NULL scene. */
int dg_scene_bsp_depth(const dg_scene *s);

/* ---- misc ----------------------------------------------------------------------------------------------------- */
const char *dg_last_error(void); /* thread-local message of the last failing call */
/* "doomgpu <release> (gfx950; ABI <n>)".  The ABI number changes whenever a struct in this header changes size or a function its
 * arguments: ABI 3 (round 3) dropped dg_timing.strips_ms and the third argument of dg_ctx_fallbacks; ABI 4 changes no signature
 * (it marks the library in which dg_version started to carry the number); functions added since (the map view, the effects, the walks,
 * the reduced readbacks, the depth frames, the label frames, the bundles, the reduced planes, the explored-map frames, the player-centred map frames, the map-object poses, the sector heights, the observation tensors, the surfaces, the screen pictures, the floor-textured map frames, the map-object markers, the sight queries) changed no struct and no signature and kept it.  A caller built against another ABI must not call on. */
const char *dg_version(void);

/* Timing of the last dg_replay_slot / submit on a slot (ms), from HIP events attached to the kernel dispatches themselves on the ctx's
 * kernel stream: setup_ms = start of the first front-end kernel .. end of the last, raster_ms = the raster launch, total_ms = both. */
typedef struct dg_timing {
    float setup_ms, raster_ms, total_ms;
    float host_ms;            /* host list generation + binning + packing of that submission (wall clock) */
    uint64_t n_spans, n_frames, covered_pixels;
    uint64_t n_walls, n_planes, list_bytes; /* drawn records / visplanes, bytes of lists copied to HBM */
    int32_t front_end;        /* DG_FE_HOST, DG_FE_DEVICE or DG_FE_DEVICE_SEGS (DG_FE_MAP, DG_FE_DEPTH, DG_FE_LABELS, DG_FE_BUNDLE, DG_FE_MAP_EXPLORED, DG_FE_MAP_EGO, DG_FE_MAP_FLOOR): what that submission actually used; with DG_FE_DEVICE setup_ms is
                                 the column walk (dg_fe_columns, dg_fe_gaps, dg_fe_scan, dg_fe_scatter), n_walls = wall records,
                                 n_planes = sprites, covered_pixels is not tracked (0) */
} dg_timing;
int dg_slot_timing(dg_ctx *ctx, int slot, dg_timing *out);

#ifdef __cplusplus
}
#endif
#endif
