// scene.hpp — immutable world data for the rasteriser, flattened for cache-friendly host walks and for HBM upload.
//
// Host-side equivalent of what the reference keeps in Rc graphs: Map (src/map/mod.rs:34-44), Palette
// (src/graphics/palette.rs), Textures/Pictures (src/graphics/textures.rs, pictures.rs), Flats (flats.rs),
// Sprites (sprites.rs) and the spawn-state view of MapObjects (src/map_objects.rs:25-50).  Everything the
// reference looks up by String per seg per frame (textures.rs:155-158, flats.rs:92-111) is resolved to an
// integer id once, here.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/doomgpu.h"
#include "fs_frame.h"
#include "light_fx.h"
#include "mobj_fx.h"
#include "walk_core.h"

namespace dg {

struct BitmapInfo {          // reference Bitmap (src/graphics/bitmap.rs:11-15): [y][x] Option<u8>
    int32_t w = 0, h = 0;
    uint32_t texel_off = 0;  // into Scene::texel_idx / texel_opq, column-major: off + x*h + y
    uint32_t has_holes = 0;  // any None texel
    int16_t top_offset = 0;  // pictures only (pictures.rs:26)
    int16_t left_offset = 0;
};

struct SectorRec {
    int16_t floor_h, ceil_h, light;
    int16_t special;                // special_type (SECTORS +22), read by the light effects
    int32_t floor_flat, ceil_flat;  // flat id when not animated (>= 0), FLAT_MISSING if the lump does not exist
    int32_t floor_anim, ceil_anim;  // index into Scene::anim (or -1)
    uint8_t floor_sky, ceil_sky;    // name contains "SKY"
    uint8_t ceil_tex_sky;           // sector.ceiling_texture.contains("SKY") (segs.rs:463-469) — same string as ceil_sky
    uint8_t pad2;
};
struct SidedefRec {
    float xoff, yoff;
    int32_t upper, lower, middle;   // bitmap id, TEX_NONE for "-", TEX_UNKNOWN if Textures::get would panic
    int32_t sector;
};
struct LinedefRec { int32_t v1, v2; int16_t flags; int16_t special; int32_t front, back; };   // special: special_type (linedefs.rs), read by the wall scroll
struct SegRec { int32_t v1, v2, linedef; int16_t offset; uint8_t direction; uint8_t pad; };
struct SubSectorRec { int32_t first, count; };
struct NodeRec {
    float x, y, dx, dy;
    int16_t rchild, lchild;
    float bb[2][4];   // [0] = right child, [1] = left child: min x, min y, max x, max y over the seg vertices of the subtree
                      // (computed at load from the segs themselves, not the NODES lump's boxes, which the reference ignores)
};
struct SpriteFrameRec { int32_t rotate; int32_t bitmap[8]; };     // sprites.rs:20-23 (= FsSpriteFrame, fs_core.h)
static_assert(sizeof(SpriteFrameRec) == sizeof(FsSpriteFrame), "SpriteFrameRec / FsSpriteFrame");
struct MapObjectRec {                                            // map_objects.rs:11-17, renderer-visible part
    float x, y, angle;
    int32_t sprite_frame;   // index into Scene::sprite_frames, -1 = state S_NULL (skipped: renderer/map_objects.rs:37)
    int32_t full_bright;
    int32_t sector;         // get_sector_from_vertex(position) as loaded; a view's pose (dg_view_poses) moves the object and derives it again
};
struct AnimList { int32_t n; int32_t flat[4]; };
struct Scene;

// The wall effects of a scene (dg_scene_set_wall_effects) as fs_core.h applies them: flags, and per seg its scroll count and
// animation lists (fs_seg_fx), the lists over bitmap ids.  flags 0: both tables empty, nothing changes.  A dg_ctx keeps the copy it uploaded.
struct WallFx {
    uint32_t flags = 0;
    std::vector<FsSegFx> seg;
    std::vector<FsAnim> lists;
    bool on() const { return flags != 0; }
};

// The light effects of a scene (dg_scene_set_light_effects) as light_fx.h evaluates them: flags, seed, one record per
// effect sector, the flash / fire tables, and per sector its record (-1: none).  flags 0: all empty.  A dg_ctx keeps the copy it uploaded.
struct LightFx {
    uint32_t flags = 0;
    uint64_t seed = 0;
    std::vector<LfxRec> recs;
    std::vector<uint32_t> tab;
    std::vector<int32_t> rec_of;
    bool on() const { return flags != 0 && !recs.empty(); }
    bool fits(const Scene &sc) const;               // on(), and set on a scene with sc's sectors: rec_of indexes them
    int16_t level(size_t rec, float timestamp) const { return lfx_level(recs[rec], tab.data(), seed, fs_tics(timestamp)); }
};

// The map-object thinkers of a scene (dg_scene_set_mobj_thinkers) as mobj_fx.h evaluates them: the live chains' steps,
// one record per driven thing type, per map object its type (-1: not driven), the driven objects, and the events.  flags 0: all empty.
// A dg_ctx keeps the copy it uploaded.
struct MobjFx {
    uint32_t flags = 0;
    std::vector<MfxStep> steps;
    std::vector<MfxChain> chains;
    std::vector<MfxType> types;
    std::vector<int32_t> type_of;
    std::vector<uint32_t> driven;
    std::vector<MfxEvent> events;
    bool on() const { return flags != 0 && !driven.empty(); }
    bool fits(const Scene &sc) const;               // on(), and set on a scene with sc's map objects: type_of indexes them
    int32_t value(size_t mobj, float timestamp) const {
        return mfx_value(types[(size_t)type_of[mobj]], events.data(), (uint32_t)events.size(), chains.data(), steps.data(), fs_tics(timestamp));
    }
};

// The three opt-in effects of a scene as one bundle: Scene::fx is what the setters last left, a dg_ctx draws with the copy it took at
// dg_upload_scene, and the host walker takes a pointer to either (frontend.hpp).
struct SceneFx {
    WallFx wall;
    LightFx light;
    MobjFx mobj;
};

enum : int32_t { TEX_NONE = -1, TEX_UNKNOWN = -2, FLAT_MISSING = -2 };

struct Scene {
    std::vector<uint8_t> wad;
    std::string map_name;
    // map
    std::vector<float> vx, vy;
    std::vector<SectorRec> sectors;
    std::vector<SidedefRec> sidedefs;
    std::vector<LinedefRec> linedefs;
    std::vector<SegRec> segs;
    std::vector<SubSectorRec> subsectors;
    std::vector<NodeRec> nodes;
    std::vector<MapObjectRec> mobjs;
    std::vector<int16_t> mobj_type;                 // per map object its thing type (doomednum), read by the map-object thinkers
    float start_x = 0, start_y = 0, start_angle = 0;
    // Map::bounding_box (src/map/mod.rs:59-64, src/geometry.rs:11-28): both vertices of every linedef, in LINEDEFS order
    float map_left = 3.40282347e38f, map_top = 3.40282347e38f, map_right = -3.40282347e38f, map_bottom = -3.40282347e38f;
    bool has_start = false;
    bool may_panic = false;                         // some sidedef texture / sector flat lookup would panic in the reference when reached
    // graphics
    uint8_t palette[768];
    std::vector<BitmapInfo> bitmaps;
    std::vector<std::string> bitmap_names;          // "T:<texture>" / "P:<picture>[:M]"
    std::vector<uint8_t> texel_idx, texel_opq;      // column-major planes
    std::vector<std::string> flat_names;            // requested names, verbatim
    std::vector<uint8_t> flat_sky;                  // per flat: name contains "SKY"
    std::vector<uint8_t> flat_pool;                 // 4096 B each, [y][x]
    std::vector<AnimList> anim;
    std::vector<SpriteFrameRec> sprite_frames;
    std::vector<std::string> sprite_frame_keys;     // "SPRT<frame>"
    int32_t sky_bitmap = TEX_UNKNOWN;
    std::vector<int32_t> pictures;                  // screen pictures (dg_scene_use_picture): the handle indexes this, the entry is a bitmap id
    uint64_t revision = 0;                         // bumped by the mutable-state setters
    std::vector<int16_t> wad_light;                 // per sector its level as the WAD holds it (the light effects' max and surrounding min)
    // as last set by set_wall_effects, set_light_effects and set_mobj_thinkers / mobj_event (dg_build_lists, dg_scene_sector_lights_at and
    // dg_scene_mobj_states_at read it)
    SceneFx fx;
    std::vector<dg_map_marker> markers;             // the map frames' marker table (dg_scene_set_map_markers): one per map object, or empty
    // The per-seg / per-sprite inputs of fs_core.h, flattened (rebuild_fs_tables: at load and whenever bitmaps or sprite frames are added):
    // what the host walker reads per seg and what dg_upload_scene copies to the GPU for DG_FE_DEVICE_SEGS.
    std::vector<FsSeg> fs_segs;                     // one per seg
    std::vector<uint16_t> fs_seg_leaf;              // subsector of every seg
    std::vector<FsSector> fs_sectors;
    std::vector<FsHeights> fs_heights;               // the sectors' heights as loaded, compact: what a view's height row starts as (view_rows_core.h)
    std::vector<FsFlats> fs_flats;                  // the sectors' flats as loaded, as handles: what a view's flat row starts as (view_rows_core.h)
    std::vector<int32_t> fs_seg_side;               // front sidedef of every seg (-1: none): what a view's sidedef entries are searched by
    std::vector<FsAnim> fs_anims;
    std::vector<FsBitmap> fs_bitmaps;
    std::vector<FsMobj> fs_mobjs;
    // BSP tables of the device seg walk (fs_frame.h): per node its partition and the seg counts of its subtrees; per leaf its ancestors,
    // root first (node | lies-in-the-LEFT-subtree << 31).  fs_ok: the map is a proper tree whose leaves partition the segs they
    // reference — otherwise (and for maps in which a texture / flat lookup would panic) only the host walker is used.
    std::vector<FsAnc> fs_anc;
    std::vector<uint32_t> fs_anc_off, fs_leaf_first;
    bool fs_ok = false;
    // The BSP as walk_core.h descends it (dg_walk_*): per node its partition and children, per leaf its floor height or
    // none, by the rule of sector_from_vertex.  Built once at load; dg_ctx_locate_walks uploads them.
    std::vector<WalkNode> walk_nodes;
    std::vector<WalkLeaf> walk_leaves;
    std::vector<int32_t> walk_leaf_sector;          // per leaf the sector that rule names (-1: none): what the pose rows' descent ends in (mobj_pose_core.h)
    void build_walk_tables();
    const FsSpriteFrame *sprite_frames_fs() const { return reinterpret_cast<const FsSpriteFrame *>(sprite_frames.data()); }
    void rebuild_fs_tables();
    void commit_new_frames(size_t frames_before);   // sprite frames were added since: a new revision, and rebuild_fs_tables

    // lookups used by the C-ABI
    int texture_id(const std::string &name) const;                               // Textures::get
    int flat_id(const std::string &name, float timestamp) const;                 // Flats::get_animated; sky => -(id+1)... see .cpp
    int sprite_bitmap_id(const std::string &sprite, uint8_t frame, uint8_t rotation) const;
    int sector_from_vertex(float x, float y) const;                              // renderer/bsp.rs:9-44
    int find_or_add_sprite_frame(const std::string &sprite, uint8_t frame, std::string &err);
    // dg_scene_use_texture / dg_scene_use_flat: the bitmap id of Textures::get(name), decoded and appended when new
    // (TEX_NONE for "-", TEX_UNKNOWN with err for an unknown name); the flat handle (fs_core.h) of Flats::get_animated(name), its lump —
    // or every member of its animation list — loaded when new (-1 with err when a lump is missing).
    int use_texture(const std::string &name, std::string &err);
    int use_flat(const std::string &name, std::string &err);
    // dg_scene_use_picture: the handle of Pictures::get(name) — the lump of that name anywhere in the WAD, decoded as the
    // loader decodes patches and sprites and appended when the scene does not hold it yet (-1 with err when there is no such lump or it
    // does not decode).  The same name gives the same handle.
    int use_picture(const std::string &name, std::string &err);
    bool is_wall_texture(int32_t id) const { return id >= 0 && (size_t)id < bitmap_names.size() && bitmap_names[(size_t)id].compare(0, 2, "T:") == 0; }
    bool is_flat_handle(int32_t h) const {
        if (h < 0 || (h & FS_FLAT_MISSING)) return false;
        const size_t i = (size_t)(h & FS_FLAT_INDEX);
        return h & FS_FLAT_ANIM ? i < anim.size() : i < flat_names.size() && ((h & FS_FLAT_SKY) != 0) == (flat_sky[i] != 0);
    }
    int set_wall_effects(uint32_t flags, std::string &err);                    // DG_OK, or DG_ERR_INVALID / DG_ERR_WAD with err
    int wall_texture_id(const std::string &name, float timestamp) const;       // texture_id after animation (DG_WALL_ANIMATE)
    int set_light_effects(uint32_t flags, uint64_t seed, std::string &err);    // DG_OK, or DG_ERR_INVALID with err
    int set_mobj_thinkers(uint32_t flags, const dg_state_rec *states, int n_states, const dg_mobj_info_rec *infos, int n_infos,
                          std::string &err);                                   // DG_OK, or DG_ERR_INVALID / DG_ERR_WAD with err
    int mobj_event(int what, float timestamp, std::string &err);               // DG_OK, or DG_ERR_INVALID with err
};

inline bool LightFx::fits(const Scene &sc) const { return on() && rec_of.size() == sc.sectors.size(); }
inline bool MobjFx::fits(const Scene &sc) const { return on() && type_of.size() == sc.mobjs.size(); }

// The lines of one 2-D map frame (Game::render with viewing_map, src/game.rs:229-308) in draw order: every linedef without DONTDRAW, then
// (view != nullptr) the player arrow's three lines P->E, R->E, L->E.  DG_ERR_INVALID for a frame under 40 x 40 or over 16384 x 16384,
// or an arrow endpoint beyond +-2^24 after the transform.  view's trig must be filled (fill_view_trig).
int map_frame_lines(const Scene &sc, int W, int H, const dg_view *view, std::vector<dg_map_line> &out, std::string &err);
// The arrow's three lines alone (what changes from one map frame to the next), with the same checks.
int map_arrow_lines(const Scene &sc, int W, int H, const dg_view &view, dg_map_line out[3], std::string &err);

// Returns nullptr and fills err on any condition where the reference's loaders panic.
Scene *load_scene_from_wad(const uint8_t *wad, size_t len, const char *map_name, std::string &err);

}  // namespace dg
