// frontend.cpp — host list generation: BSP walk, seg classification, projection, per-column clip arrays,
// visplane assembly, sprite projection/clipping/sorting.  No pixel work happens here; see frontend.hpp.
//
// Arithmetic contract: IEEE f32, no contraction (-ffp-contract=off), Rust `as` casts via rust_num.h.
#include "frontend.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "fs_core.h"
#include "rust_num.h"

namespace dg {

namespace {

const float kEye = 41.0f;  // PLAYER_EYE_HEIGHT, src/renderer/constants.rs:3

// (V2, Seg2, clip_to_viewport, project, ... : fs_core.h — shared with the GPU's per-seg kernels)
inline V2 sub(V2 p, V2 q) { return v2_sub(p, q); }
inline V2 rot(V2 v, float c, float s) { return v2_rot(v, c, s); }

enum : uint8_t { ST_SOLID, ST_TWOSIDED, ST_DRAWN, ST_MAPOBJECT };   // bitmap_render.rs:11-17

}  // namespace

struct FrameArena::Rec {                                             // bitmap_render.rs:29-45
    Seg2 line;
    float start_offset, bottom_height, top_height;
    float min_x, max_x;            // of line.a.x / line.b.x, for is_behind_vertex
    int32_t start_x, end_x, bitmap;
    uint32_t first_col, n_cols;
    int32_t out_index;             // index in arena.renders once emitted, else -1
    int16_t light, offset_x, offset_y;
    uint8_t state, ext_bottom, ext_top, draw_ceiling;
    int16_t sort_key;              // map objects: line.start.x as i16 (bitmap_render.rs:168-174)
    uint32_t owner;                // host-list mode: the seg or map object that made the record (doomgpu.h: class << 16 | index)
};

FrameArena::FrameArena() : recs(new std::vector<Rec>()) {}
FrameArena::~FrameArena() { delete recs; }

FrameConsts make_consts(int W, int H) {
    FrameConsts k;
    k.ARC = 200.0f / 240.0f;
    k.GSW = (float)W / k.ARC;
    k.GCFX = k.GSW / 2.0f;
    k.CFX = (float)W / 2.0f;
    k.CFY = (float)H / 2.0f;
    k.W = W;
    k.H = H;
    return k;
}

DevWallRec make_wall_rec(const BitmapInfo &bi, float lsx, float lsy, float lex, float ley, float start_offset, int32_t start_x, int32_t end_x,
                         float bottom_height, float top_height, int16_t offset_x, int16_t offset_y, int16_t light_level) {
    const FsBitmap fb{bi.texel_off, (int16_t)bi.w, (int16_t)bi.h, bi.top_offset, (uint16_t)bi.has_holes};
    return fs_wall_rec(fb, lsx, lsy, lex, ley, start_offset, start_x, end_x, bottom_height, top_height, offset_x, offset_y, light_level);
}

void fill_view_trig(dg_view &v) {
    if (v.trig_valid) return;
    v.cos_a = cosf(v.angle);
    v.sin_a = sinf(v.angle);
    v.cos_na = cosf(-v.angle);
    v.sin_na = sinf(-v.angle);
    v.trig_valid = 1;
}

namespace {

using Rec = FrameArena::Rec;

struct PlaneBuilder {          // one open visplane of SidedefVisPlanes (sidedef_visplanes.rs:7-17)
    bool used = false;
    int16_t left = -1, right = -1;
    uint32_t first = 0;        // entry index in its pool
};

// Union of closed column intervals, kept sorted and merged (adjacent intervals fuse): Doom's "solidsegs", here only a
// conservative summary of horizontal_ocl used to drop records that cannot matter.
struct ColumnIntervals {
    std::vector<std::pair<int, int>> iv;
    void clear() { iv.clear(); }
    bool covers(int lo, int hi) const {
        for (const auto &r : iv) {
            if (r.first > lo) return false;
            if (r.second >= lo) return r.second >= hi;
        }
        return false;
    }
    void add(int lo, int hi) {
        size_t i = 0;
        while (i < iv.size() && iv[i].second + 1 < lo) i++;
        size_t j = i;
        while (j < iv.size() && iv[j].first <= hi + 1) { lo = std::min(lo, iv[j].first); hi = std::max(hi, iv[j].second); j++; }
        iv.erase(iv.begin() + (ptrdiff_t)i, iv.begin() + (ptrdiff_t)j);
        iv.insert(iv.begin() + (ptrdiff_t)i, std::make_pair(lo, hi));
    }
};

struct Walker {
    const Scene &sc;
    const FrameConsts k;
    const dg_view &view;
    FrameArena &A;
    std::vector<Rec> &recs;
    std::string &err;
    V2 ppos;
    float player_height;
    int status = DG_OK;
    bool parts_mode = false;      // record FePart / FeSprite instead of walking columns
    ColumnIntervals solid_cols;   // columns spanned by full-height solid parts so far
    uint32_t n_floor_planes_marker = 0;
    // visplanes carry a pool tag in the top bit of first_entry until finalisation
    static constexpr uint32_t kCeilPool = 0x80000000u;

    const dg_view_state *state = nullptr;   // this view's game-state snapshot (light levels, mobj states) on top of the scene's
    const WallFx *fx = nullptr;             // the wall effects to draw with (nullptr: none)
    const LightFx *lfx = nullptr;           // the light effects to draw with (nullptr: none)
    const MobjFx *mfx = nullptr;            // the map-object thinkers to draw with (nullptr: none)
    const dg_view_poses *poses = nullptr;   // where this view's map objects are (nullptr: where the scene has them)
    const FsHeights *hrow = nullptr;        // this view's sector heights, [sector] (nullptr: the scene's, as loaded)
    bool has_sf = false;                    // this view brings surfaces: sf answers for its sidedefs and flats (and hrow is set)
    FsViewSurfaces sf{};
    uint32_t cur_owner = 0;                 // owner tag of the seg / map object being processed (host-list mode)
    static constexpr int32_t kNoOverride = INT32_MIN;

    // sector.light_level / map object state as the reference's thinkers would have left them before this frame
    // (src/lights.rs:47-259, src/map_objects.rs:63-121): the view's snapshot entry if there is one, else the light effect's level
    //  or the map-object thinker's state (§8d), else the scene's value.  The arena's two rows hold what overrides the
    // scene: the effects' values, every effect sector and driven object once per frame, then the view's entries on top.
    Walker(const Scene &s, int W, int H, const dg_view &v, FrameArena &a, std::string &e, const ViewInputs &in, const SceneFx *f)
        : sc(s), k(make_consts(W, H)), view(v), A(a), recs(*a.recs), err(e), state(in.state), fx(f && f->wall.on() ? &f->wall : nullptr),
          lfx(f && f->light.fits(s) ? &f->light : nullptr), mfx(f && f->mobj.fits(s) ? &f->mobj : nullptr), poses(in.poses) {
        const dg_view_sectors *const vs = in.sectors;
        const dg_view_surfaces *const vf = in.surfaces;
        ppos = V2{v.x, v.y};
        player_height = v.floor_height + kEye;
        if (A.light_row.size() != sc.sectors.size()) A.light_row.assign(sc.sectors.size(), kNoOverride);
        if (A.mobj_row.size() != sc.mobjs.size()) A.mobj_row.assign(sc.mobjs.size(), kNoOverride);
        if (lfx)
            for (size_t r = 0; r < lfx->recs.size(); r++) A.light_row[lfx->recs[r].sector] = lfx->level(r, v.timestamp);
        if (mfx)
            for (uint32_t i : mfx->driven) A.mobj_row[i] = mfx->value(i, v.timestamp);
        if (poses && !resolve_view_poses(sc, *poses, A.poses)) { status = DG_ERR_INVALID; err = "view poses: map object index out of range"; }
        if (vs) {                                                    // the scene's heights with the view's entries on top, a row of this frame alone
            const unsigned bad = resolve_view_sectors(sc, *vs, A.heights);
            A.height_row.assign(sc.fs_heights.begin(), sc.fs_heights.end());
            for (const dg_sector_heights &h : A.heights.out) sector_row_place(A.height_row.data(), h.sector, h.floor_height, h.ceiling_height);
            A.heights.release();
            hrow = A.height_row.data();
            if (bad) { status = DG_ERR_INVALID; err = view_sectors_error(bad); }
        }
        if (vf) {                                                    // likewise the flats, and the sorted sidedef entries fs_seg searches
            const unsigned bad = resolve_view_surfaces(sc, fx, *vf, 0, A.sides, A.flats);
            A.flat_row.assign(sc.fs_flats.begin(), sc.fs_flats.end());
            for (const FlatEntry &e : A.flats.out) flat_row_place(A.flat_row.data(), e.sector, e.flats);
            if (!hrow) { A.height_row.assign(sc.fs_heights.begin(), sc.fs_heights.end()); hrow = A.height_row.data(); }   // (surfaces read heights through the row, as on the device)
            sf = FsViewSurfaces{A.flat_row.data(), A.sides.out.data(), (uint32_t)A.sides.out.size(), sc.fs_seg_side.data()};
            has_sf = true;
            if (bad) { status = DG_ERR_INVALID; err = view_surfaces_error(bad); }
        }
        if (!state) return;
        const unsigned bad = apply_view_state(sc, *state, [&](size_t i, int32_t level) { A.light_row[i] = level; }, [&](size_t i, int32_t val) { A.mobj_row[i] = val; });
        if (bad) { status = DG_ERR_INVALID; err = bad & 2u ? "view state: map object or sprite frame index out of range" : "view state: sector index out of range"; }
    }
    ~Walker() {                                                      // the entries written go back to "no override"
        if (lfx)
            for (const LfxRec &r : lfx->recs) A.light_row[r.sector] = kNoOverride;
        if (mfx)
            for (uint32_t i : mfx->driven) A.mobj_row[i] = kNoOverride;
        if (state) apply_view_state(sc, *state, [&](size_t i, int32_t) { A.light_row[i] = kNoOverride; }, [&](size_t i, int32_t) { A.mobj_row[i] = kNoOverride; });
        if (poses) A.poses.release();
    }
    // MapObject.position / .angle and get_sector_from_vertex(position) as draw_map_objects reads them for this frame
    // (renderer/map_objects.rs:55,74,99-116): the view's pose if it has one for the object, else the scene's row.
    FsMobj mobj_placed(size_t i) const {
        const int32_t at = poses ? A.poses.of[i] : -1;
        if (at < 0) return sc.fs_mobjs[i];
        const dg_mobj_pose &p = A.poses.out[(size_t)at];
        return FsMobj{p.x, p.y, p.angle, sc.sector_from_vertex(p.x, p.y)};
    }
    int16_t sector_light(int sector) const {
        const int32_t v = A.light_row[(size_t)sector];
        return v != kNoOverride ? (int16_t)v : sc.sectors[(size_t)sector].light;
    }
    void mobj_state(size_t i, int32_t &sprite_frame, int32_t &full_bright) const {
        const MapObjectRec &m = sc.mobjs[i];
        if (A.mobj_row[i] != kNoOverride) mfx_decode(A.mobj_row[i], sprite_frame, full_bright);
        else { sprite_frame = m.sprite_frame; full_bright = m.full_bright; }
    }

    int fail(const std::string &m) {
        if (status == DG_OK) { status = DG_ERR_RENDER; err = m; }
        return status;
    }
    int fail_parts(const std::string &m) {                          // parts mode cannot tell: let the host list path decide
        if (status == DG_OK) { status = kPartsUnsupported; err = m; }
        return status;
    }
    int fail_fs(int32_t code) { return code == FS_FAIL_PARTS ? fail_parts(fs_message(code)) : fail(fs_message(code)); }   // an FS_* failure of fs_core.h

    void occlude(int x) {                                           // segs.rs:113-117
        A.hor_ocl[(size_t)x] = 1;
        A.floor_ocl[(size_t)x] = (int16_t)((int16_t)k.H / 2);
        A.ceil_ocl[(size_t)x] = (int16_t)((int16_t)k.H / 2);
    }

    void plane_add(PlaneBuilder &p, std::vector<int16_t> &pool, int16_t x, int16_t top, int16_t bottom) {
        if (!p.used) {                                              // sidedef_visplanes.rs:60-83
            p.left = x;
            p.first = (uint32_t)(pool.size() / 2);
            p.used = true;
        } else {
            for (int g = p.right + 1; g < x; g++) { pool.push_back(0); pool.push_back(0); }  // Visplane::new zero fill
        }
        p.right = x;
        pool.push_back(top);
        pool.push_back(bottom);
    }
    void plane_flush(PlaneBuilder &p, bool ceil, int flat, int16_t height, int16_t light) {
        if (!p.used) return;
        dg_visplane v;
        v.flat = flat; v.height = height; v.light_level = light; v.left = p.left; v.right = p.right;
        v.first_entry = p.first | (ceil ? kCeilPool : 0u);
        A.visplanes.push_back(v);
        p.used = false;
    }

    struct Flags { bool only_occlusions, lower, upper, draw_ceiling, two_sided_mid; };   // segs.rs:53-59

    static Rec make_rec(const Seg2 &line, uint8_t state) {          // what every record starts from
        Rec r;
        std::memset(&r, 0, sizeof r);
        r.line = line;
        r.min_x = std::fmin(line.a.x, line.b.x); r.max_x = std::fmax(line.a.x, line.b.x);
        r.state = state;
        r.out_index = -1;
        return r;
    }

    void emit_draw(Rec &r) {
        if (r.out_index < 0) {
            dg_bitmap_render o;
            std::memset(&o, 0, sizeof o);
            o.bitmap = r.bitmap; o.light_level = r.light; o.offset_x = r.offset_x; o.offset_y = r.offset_y;
            o.line_start_x = r.line.a.x; o.line_start_y = r.line.a.y; o.line_end_x = r.line.b.x; o.line_end_y = r.line.b.y;
            o.start_offset = r.start_offset; o.start_x = r.start_x; o.end_x = r.end_x;
            o.bottom_height = r.bottom_height; o.top_height = r.top_height;
            o.first_column = r.first_col; o.n_columns = r.n_cols;
            r.out_index = (int32_t)A.renders.size();
            A.renders.push_back(o);
            A.owners.push_back(r.owner);
        }
        A.order.push_back(dg_draw_cmd{0u, (uint32_t)r.out_index});
    }

    // Segs::process_sidedef, segs.rs:121-350.  s: the seg's SideDefDetails (segs.rs:42-51).  The geometry and the reference's panics are
    // fs_core.h's in both modes: parts mode takes the whole record (fs_part), list mode the part of it that comes before the fill.
    void process_sidedef(const FsSegOut &s, const FsCall &call) {
        const int H = k.H;
        const Flags f{(call.flags & FEP_ONLY_OCCL) != 0, (call.flags & FEP_LOWER) != 0, (call.flags & FEP_UPPER) != 0, (call.flags & FEP_DRAW_CEILING) != 0,
                      (call.flags & FEP_TWO_SIDED_MID) != 0};
        FePart p;
        FsPartGeom g{};
        if (parts_mode) std::memset(&p, 0, sizeof p);
        const int32_t st = parts_mode ? fs_part(k, s, call, sc.fs_bitmaps.data(), sc.flat_sky.data(), view.floor_height, p) : fs_part_geom(k, s, call, g);
        if (st == FS_SKIP) return;
        if (st != FS_OK) { fail_fs(st); return; }
        const int sx = parts_mode ? p.sx : g.bot.sx, ex = parts_mode ? p.ex : g.bot.ex;
        // Columns that an earlier full-height solid part spans are horizontally occluded whatever that part's own
        // visibility was (segs.rs:341-344 runs for every column of the part).  A part lying entirely inside them can
        // neither draw, clip, add a visplane entry nor occlude anything new (segs.rs:211,337-341): it is dropped here.
        if (solid_cols.covers(sx, ex)) return;
        if (fs_part_is_solid(call.flags) && sx <= ex) solid_cols.add(sx, ex);
        Rec r = make_rec(s.cl.line, f.two_sided_mid ? ST_TWOSIDED : ST_SOLID);
        if (parts_mode) {                                            // the per-column half runs on the GPU: record the part
            if (fs_part_wants_sky_slot(p.flags)) {
                p.sky_slot = (int32_t)A.n_sky_slots++;
                A.sky_parts.push_back((uint32_t)A.parts.size());
            }
            if (A.parts.size() >= 65535) { fail_parts("more than 65535 wall records in a frame"); return; }
            A.parts.push_back(p);
            recs.push_back(r);
            return;
        }
        const ScreenLine &bot = g.bot, &top = g.top;
        const float bottom_delta = g.bottom_delta, top_delta = g.top_delta;
        const int tex = call.tex;
        const bool full_height = !f.lower && !f.upper && !f.only_occlusions;
        const bool planes_here = !f.two_sided_mid && (full_height || f.only_occlusions);
        PlaneBuilder pb, pt;

        r.start_offset = s.cl.start_offset;
        r.bottom_height = call.bottom_height; r.top_height = call.top_height;
        r.start_x = bot.sx; r.end_x = bot.ex; r.bitmap = tex;
        r.first_col = (uint32_t)A.columns.size();
        r.light = s.light;
        fs_part_offsets(s, call, r.offset_x, r.offset_y);
        r.ext_bottom = f.lower || (!f.two_sided_mid && full_height);
        r.ext_top = f.upper || (!f.two_sided_mid && full_height);
        r.draw_ceiling = f.draw_ceiling;
        r.owner = cur_owner;

        const int16_t hm1 = (int16_t)(H - 1);
        for (int x = bot.sx; x <= bot.ex; x++) {
            if (!A.hor_ocl[(size_t)x]) {
                int16_t bottom_y = (int16_t)f32_as_i16((float)bot.sy + ((float)x - (float)bot.sx) * bottom_delta);
                int16_t top_y = (int16_t)f32_as_i16((float)top.sy + ((float)x - (float)top.sx) * top_delta);
                int16_t fo = A.floor_ocl[(size_t)x], co = A.ceil_ocl[(size_t)x];
                int16_t cb = std::min(hm1, std::min(fo, bottom_y));
                int16_t ct = std::max((int16_t)0, std::max(co, top_y));
                bool vis = cb >= ct;
                if (vis) {
                    A.columns.push_back(dg_bitmap_column{(int16_t)x, ct, cb, bottom_y, top_y});
                    r.n_cols++;
                }
                if (planes_here && vis) {
                    bool added = false;
                    if (cb < fo && cb != hm1) { plane_add(pb, A.floor_tb, (int16_t)x, cb, fo); added = true; }
                    if (f.draw_ceiling && ct > co && ct != -1) { plane_add(pt, A.ceil_tb, (int16_t)x, co, ct); added = true; }
                    if (!added) {
                        plane_flush(pb, false, s.floor_flat, s.floor_h, s.light);
                        plane_flush(pt, true, s.ceil_flat, s.ceil_h, s.light);
                    }
                } else if (planes_here && !vis && fo > co) {        // occluded wall, open vertical gap (segs.rs:293-318)
                    if (bottom_y <= co) { plane_add(pb, A.floor_tb, (int16_t)x, co, fo); occlude(x); }
                    if (f.draw_ceiling && top_y >= fo) { plane_add(pt, A.ceil_tb, (int16_t)x, co, fo); occlude(x); }
                }
                if (!f.two_sided_mid && vis) {
                    if (f.only_occlusions) {
                        A.floor_ocl[(size_t)x] = cb;
                        if (f.draw_ceiling) A.ceil_ocl[(size_t)x] = ct;
                    }
                    if (f.lower) A.floor_ocl[(size_t)x] = ct;
                    if (f.upper) A.ceil_ocl[(size_t)x] = cb;
                }
            } else {
                plane_flush(pb, false, s.floor_flat, s.floor_h, s.light);
                plane_flush(pt, true, s.ceil_flat, s.ceil_h, s.light);
            }
            if (!f.two_sided_mid && full_height) occlude(x);
        }
        plane_flush(pb, false, s.floor_flat, s.floor_h, s.light);
        plane_flush(pt, true, s.ceil_flat, s.ceil_h, s.light);

        recs.push_back(r);
        // inline draw of solid / upper / lower parts (segs.rs:231-258)
        if (!f.two_sided_mid && !f.only_occlusions && tex >= 0 && r.n_cols > 0) emit_draw(recs.back());
    }

    static const char *fs_message(int32_t code) {
        switch (code) {
            case FS_FAIL_CLIP_X: return "Clipped line x < -0.01 (segs.rs:431-436)";
            case FS_FAIL_FLAT: return "Could not find flat lump (Flat::new unwrap, flats.rs:117)";
            case FS_FAIL_TEXTURE: return "Unknown texture (Textures::get panics, textures.rs:158)";
            case FS_FAIL_VERTICAL: return "Wall start not vertical (segs.rs:140-145)";
            case FS_FAIL_LINE_X: return "Invalid line x (segs.rs:103-111)";
            case FS_FAIL_ROTATION: return "Invalid rotation (sprites.rs:106-108)";
            case FS_FAIL_MOBJ_CLIP_X: return "Clipped line x < -0.01 (map_objects.rs:92-97)";
            case FS_FAIL_MOBJ_COLUMN: return "map object column out of range (index panic)";
            default: return "zero-sized bitmap";
        }
    }

    // Segs::process_seg, segs.rs:353-590: fs_seg (fs_core.h) classifies the seg and lists its process_sidedef calls
    void process_seg(size_t seg_index) {
        FsSeg sg = sc.fs_segs[seg_index];
        cur_owner = ((uint32_t)DG_LABEL_WALL << 16) | (uint32_t)(seg_index & 0xffffu);
        FsSegOut so;
        const int16_t light = sg.front_sector >= 0 ? sector_light(sg.front_sector) : (int16_t)0;
        if (fx && !has_sf) fs_seg_fx(sg, fx->seg[seg_index], fx->lists.data(), view.timestamp);
        const auto with_sf = [&](const auto &wfx) {                   // the device's composition: the policy first, the effects on what it answers
            return fs_seg(k, sg, sc.fs_sectors.data(), sc.fs_anims.data(), ppos, view.cos_na, view.sin_na, player_height, view.timestamp, light, so, wfx, (uint32_t)seg_index, FsRowHeights{hrow}, sf);
        };
        const int32_t st = has_sf ? (fx ? with_sf(FsFx{fx->seg.data(), fx->lists.data()}) : with_sf(FsNoFx())) : hrow ? fs_seg(k, sg, sc.fs_sectors.data(), sc.fs_anims.data(), ppos, view.cos_na, view.sin_na, player_height, view.timestamp, light, so, FsNoFx(), 0, FsRowHeights{hrow})
                                : fs_seg(k, sg, sc.fs_sectors.data(), sc.fs_anims.data(), ppos, view.cos_na, view.sin_na, player_height, view.timestamp, light, so);
        if (st == FS_SKIP) return;
        if (st != FS_OK) { fail_fs(st); return; }
        for (int i = 0; i < so.n_calls && !status; i++)
            if ((so.call_mask >> i) & 1u) process_sidedef(so, so.call[i]);
    }

    // Renderer::render_node, mod.rs:69-104 — iterative, front child first, no culling (the reference has none)
    // Can any seg inside the box (map coordinates) still matter?  No if the box lies behind the viewer or
    // outside the 90-degree frustum (clip_to_viewport rejects every seg in it), or if the screen columns it can project to
    // are all spanned by earlier full-height solid parts (every part of every seg in it would be dropped by
    // solid_cols.covers).  The column range is widened by two columns against f32 rounding of the per-seg projection;
    // boxes that straddle the viewer's depth-zero plane are always walked.
    //
    // Why two columns are enough (W <= 16384; tests/test_host_logic.py::test_subtree_cull_at_16384_columns_next_to_walls is the stress
    // case).  Past the `xmin < 1` test all four corners have view depth x >= 1.  In exact arithmetic every seg endpoint e inside the
    // box maps to a point p of the convex hull of the transformed corners, x(p) >= 1 there, and t = y / x — a ratio of affine
    // functions, monotone along any segment — takes its extremes over the hull at corners: t(p) in [tmin, tmax].  clip_to_viewport
    // (misc.rs:13-115) replaces an endpoint only by a point of the same seg on y = x or y = -x, so every endpoint that reaches
    // make_sidedef_non_vertical_line has t in [max(tmin, -1), min(tmax, 1)]: the interval projected below.  In f32: corner and
    // endpoint go through the same six operations of rot(sub(.)), each with relative error u = 2^-24, so |dx|, |dy| <= 4.3 u r with
    // r = |e - pos|; a kept endpoint has |y| <= x, i.e. r <= 1.42 x, which bounds its error in t by (|dy| + |t| |dx|) / x <= 12.3 u;
    // an intersection computed by Line::intersection (geometry.rs:56-82) adds a few more operations — 32 u = 1.9e-6 is generous.
    // sx = trunc(CFX - ARC * (GCFX * y / x)) (misc.rs:147-158) then moves by at most K * 1.9e-6 = 0.016 columns (K = ARC * GCFX <=
    // 8192) plus three roundings of values below 16384 (<= 0.003 columns): under 0.02 columns between the corner-derived bounds and
    // any endpoint's sx, before truncation.  floor() of the bounds minus / plus 2 therefore leaves a margin of more than 1.9 columns.
    bool box_matters(const float *bb) const {
        if (bb[0] > bb[2]) return false;                             // no segs below this child
        float tmin = 3.0e38f, tmax = -3.0e38f, xmin = 3.0e38f, xmax = -3.0e38f;
        for (int c = 0; c < 4; c++) {
            V2 v = rot(sub(V2{bb[(c & 1) ? 2 : 0], bb[(c & 2) ? 3 : 1]}, ppos), view.cos_na, view.sin_na);
            xmin = std::fmin(xmin, v.x); xmax = std::fmax(xmax, v.x);
            if (v.x > 0.0f) { float t = v.y / v.x; tmin = std::fmin(tmin, t); tmax = std::fmax(tmax, t); }
        }
        if (xmax < -1.0f) return false;                              // wholly behind the viewer
        if (xmin < 1.0f) return true;                                // around or next to the viewer: walk it
        if (tmin > 1.001f || tmax < -1.001f) return false;           // wholly outside the frustum (|y| <= x)
        const float K = k.ARC * k.GCFX;                              // sx = CFX - K * (y / x), misc.rs:147-158
        float lo = k.CFX - K * std::fmin(tmax, 1.0f), hi = k.CFX - K * std::fmax(tmin, -1.0f);
        int ilo = std::max(0, (int)std::floor(lo) - 2), ihi = std::min(k.W - 1, (int)std::floor(hi) + 2);
        return !solid_cols.covers(ilo, ihi);
    }

    void walk_bsp() {
        int16_t stack[256];
        const float *box[256];
        int sp = 0;
        const bool cull = !sc.may_panic;                             // a seg whose lookup would panic must be reached
        stack[sp] = (int16_t)(sc.nodes.size() - 1);
        box[sp++] = nullptr;
        while (sp > 0 && !status) {
            --sp;
            int16_t c = stack[sp];
            if (cull && box[sp] && !box_matters(box[sp])) continue;
            if (c & (int16_t)0x8000) {
                const SubSectorRec &ss = sc.subsectors[(size_t)(c & 0x7fff)];
                for (int i = 0; i < ss.count && !status; i++) process_seg((size_t)(ss.first + i));
                continue;
            }
            const NodeRec &n = sc.nodes[(size_t)c];
            V2 v1{n.x, n.y}, v2{n.x + n.dx, n.y + n.dy};
            bool is_left = left_of(ppos, Seg2{v1, v2});
            int16_t front = is_left ? n.lchild : n.rchild, back = is_left ? n.rchild : n.lchild;
            if (sp + 2 > 256) { fail("BSP deeper than 256"); return; }
            stack[sp] = back;
            box[sp++] = n.bb[is_left ? 0 : 1];
            stack[sp] = front;
            box[sp++] = n.bb[is_left ? 1 : 0];
        }
    }

    static bool behind(const Rec &r, V2 v) { return fs_behind(r.line, r.min_x, r.max_x, v); }   // is_behind_vertex, bitmap_render.rs:137-165

    // The sprite / masked-wall interleave (map_objects.rs:218-241) and draw_remaining_segs after it (segs.rs:593-597): in front of each
    // sprite of mo (far to near) go the two-sided middles behind its centre that are not drawn yet, after the last sprite the rest.
    // `segs` was reversed before (mod.rs:124): wall records go back to front.
    template <typename DrawWall, typename DrawSprite>
    void interleave(const std::vector<uint32_t> &mo, size_t n_wall_recs, DrawWall draw_wall, DrawSprite draw_sprite) {
        for (size_t i = 0; i <= mo.size(); i++) {
            const bool rest = i == mo.size();
            const Seg2 l = rest ? Seg2{} : recs[mo[i]].line;
            const V2 v{(l.a.x + l.b.x) / 2.0f, (l.a.y + l.b.y) / 2.0f};
            for (size_t ri = n_wall_recs; ri-- > 0;) {
                Rec &r = recs[ri];
                if (r.state != ST_TWOSIDED || (!rest && !behind(r, v))) continue;
                draw_wall(ri);
                r.state = ST_DRAWN;
            }
            if (!rest) draw_sprite(mo[i]);
        }
    }

    // draw_map_objects, renderer/map_objects.rs:19-241.  As in process_sidedef, the geometry and the panics are fs_core.h's in both modes.
    void map_objects() {
        const int H = k.H;
        const size_t n_wall_recs = recs.size();
        if (parts_mode) A.behind_words = (uint32_t)((n_wall_recs + 31) / 32);
        std::vector<uint32_t> mo;   // indices of map-object records in recs
        for (size_t mi = 0; mi < sc.mobjs.size(); mi++) {
            int32_t m_sprite_frame, m_full_bright;
            mobj_state(mi, m_sprite_frame, m_full_bright);
            if (m_sprite_frame < 0) continue;                         // S_NULL
            const FsMobj fm = mobj_placed(mi);
            const FsSpriteFrame &sf = sc.sprite_frames_fs()[(size_t)m_sprite_frame];
            const int16_t light = fm.sector >= 0 ? sector_light(fm.sector) : (int16_t)0;
            FsSpriteOut so;
            FsMobjGeom g{};
            if (parts_mode) std::memset(&so.sp, 0, sizeof so.sp);
            const auto placed = [&](const auto &ht) {                 // z = the sector's floor height as this view has it
                return parts_mode ? fs_mobj(k, fm, sf, sc.fs_bitmaps.data(), sc.fs_sectors.data(), ppos, view.angle, view.cos_na, view.sin_na, player_height, m_full_bright, light, so, ht)
                                  : fs_mobj_geom(k, fm, sf, sc.fs_bitmaps.data(), sc.fs_sectors.data(), ppos, view.angle, view.cos_na, view.sin_na, player_height, m_full_bright, light, g, ht);
            };
            const int32_t st = hrow ? placed(FsRowHeights{hrow}) : placed(FsOwnHeights());
            if (st == FS_SKIP) continue;
            if (st != FS_OK) { fail_fs(st); return; }
            Rec r = make_rec(parts_mode ? so.line : g.cl.line, ST_MAPOBJECT);
            r.sort_key = (int16_t)(parts_mode ? so.sort_key : g.sort_key);
            mo.push_back((uint32_t)recs.size());
            if (parts_mode) {                                         // the per-column half runs on the GPU: record the sprite
                r.first_col = (uint32_t)A.sprites.size();             // first_col: index into A.sprites
                // which wall records clip this sprite (the ones NOT behind its centre, map_objects.rs:138-140)
                const size_t row = A.behind.size();
                A.behind.resize(row + A.behind_words, 0u);
                for (size_t ri = 0; ri < n_wall_recs; ri++)
                    if (behind(recs[ri], so.centre)) A.behind[row + (ri >> 5)] |= 1u << (ri & 31);
                so.sp.behind_off = (uint32_t)row;
                A.sprites.push_back(so.sp);
                recs.push_back(r);
                continue;
            }
            const V2 vpv = g.vpv;
            const ScreenLine &bot = g.bot, &top = g.top;
            const int x0 = g.x0, x1 = g.x1;
            for (int x = x0; x < x1; x++) { A.top_clip[(size_t)x] = -1; A.bottom_clip[(size_t)x] = (int16_t)H; }
            if (x0 < x1) {
                for (size_t ri = 0; ri < n_wall_recs; ri++) {         // :135-166 (only x in [x0,x1) is ever read back)
                    const Rec &r = recs[ri];
                    if (r.n_cols == 0 || behind(r, vpv)) continue;
                    bool solid = r.state == ST_SOLID;
                    if (solid && !r.ext_bottom && !r.ext_top) continue;
                    const dg_bitmap_column *c0 = &A.columns[r.first_col], *c1 = c0 + r.n_cols;
                    const dg_bitmap_column *c = std::lower_bound(c0, c1, x0, [](const dg_bitmap_column &q, int v) { return q.x < v; });
                    for (; c < c1 && c->x < x1; ++c) {
                        size_t x = (size_t)c->x;
                        if (solid) {
                            if (r.ext_bottom) A.bottom_clip[x] = std::min(A.bottom_clip[x], c->clipped_top_y);
                            if (r.ext_top) A.top_clip[x] = std::max(A.top_clip[x], c->clipped_bottom_y);
                        } else {                                       // ST_TWOSIDED (nothing is ST_DRAWN yet)
                            if (r.draw_ceiling) A.top_clip[x] = std::max(A.top_clip[x], c->top_y);
                            A.bottom_clip[x] = std::min(A.bottom_clip[x], c->bottom_y);
                        }
                    }
                }
            }
            r.start_offset = g.cl.start_offset;
            r.bottom_height = g.bottom_height; r.top_height = g.top_height;
            r.start_x = bot.sx; r.end_x = bot.ex; r.bitmap = g.bitmap;
            r.first_col = (uint32_t)A.columns.size();
            r.light = g.light;
            r.owner = ((uint32_t)DG_LABEL_MOBJ << 16) | (uint32_t)(mi & 0xffffu);
            const float bottom_delta = fs_slope(bot), top_delta = fs_slope(top);
            for (int x = x0; x < x1; x++) {
                int16_t bottom_y = (int16_t)f32_as_i16((float)bot.sy + ((float)x - (float)bot.sx) * bottom_delta);
                int16_t top_y = (int16_t)f32_as_i16((float)top.sy + ((float)x - (float)top.sx) * top_delta);
                int16_t ct = std::max((int16_t)0, std::max(top_y, A.top_clip[(size_t)x]));
                int16_t cb = std::min((int16_t)(H - 1), std::min(bottom_y, A.bottom_clip[(size_t)x]));
                A.columns.push_back(dg_bitmap_column{(int16_t)x, ct, cb, bottom_y, top_y});
                r.n_cols++;
            }
            recs.push_back(r);
        }
        // sort() is stable ascending on the key, then reverse()  (map_objects.rs:216-217)
        std::stable_sort(mo.begin(), mo.end(), [&](uint32_t p, uint32_t q) { return recs[p].sort_key < recs[q].sort_key; });
        std::reverse(mo.begin(), mo.end());

        if (parts_mode) {                                            // "draw" = the record's place in the sequence
            uint32_t seq = 0;
            interleave(mo, n_wall_recs, [&](size_t ri) { A.parts[ri].seq = seq++; }, [&](uint32_t mi) { A.sprites[recs[mi].first_col].seq = seq++; });
        } else {
            const auto draw = [&](size_t i) { if (recs[i].bitmap >= 0 && recs[i].n_cols > 0) emit_draw(recs[i]); };   // (a sprite always has a bitmap)
            interleave(mo, n_wall_recs, draw, draw);
        }
    }
};

}  // namespace

int build_frame_lists(const Scene &sc, int W, int H, const dg_view &view, FrameArena &A, dg_frame_lists &out, std::string &err, const ViewInputs &in, const SceneFx *fx) {
    if (W <= 0 || H <= 0 || W > 16384 || H > 16384) { err = "bad frame size"; return DG_ERR_INVALID; }
    A.renders.clear(); A.owners.clear(); A.columns.clear(); A.visplanes.clear(); A.plane_tb.clear(); A.order.clear();
    A.recs->clear(); A.floor_tb.clear(); A.ceil_tb.clear();
    A.hor_ocl.assign((size_t)W, 0);                                  // Segs::new, segs.rs:97-99
    A.floor_ocl.assign((size_t)W, (int16_t)H);
    A.ceil_ocl.assign((size_t)W, (int16_t)-1);
    A.top_clip.resize((size_t)W);
    A.bottom_clip.resize((size_t)W);

    Walker wk(sc, W, H, view, A, err, in, fx);
    if (wk.status) return wk.status;
    wk.walk_bsp();
    if (wk.status) return wk.status;
    // visplanes are drawn after all inline walls, in push order (mod.rs:122)
    const uint32_t n_floor_entries = (uint32_t)(A.floor_tb.size() / 2);
    A.plane_tb.reserve(A.floor_tb.size() + A.ceil_tb.size());
    A.plane_tb.insert(A.plane_tb.end(), A.floor_tb.begin(), A.floor_tb.end());
    A.plane_tb.insert(A.plane_tb.end(), A.ceil_tb.begin(), A.ceil_tb.end());
    for (uint32_t i = 0; i < A.visplanes.size(); i++) {
        dg_visplane &v = A.visplanes[i];
        if (v.first_entry & Walker::kCeilPool) v.first_entry = (v.first_entry & ~Walker::kCeilPool) + n_floor_entries;
        A.order.push_back(dg_draw_cmd{1u, i});
    }
    wk.map_objects();
    if (wk.status) return wk.status;

    out.view = view;
    out.renders = A.renders.data(); out.n_renders = (uint32_t)A.renders.size();
    out.columns = A.columns.data(); out.n_columns = (uint32_t)A.columns.size();
    out.visplanes = A.visplanes.data(); out.n_visplanes = (uint32_t)A.visplanes.size();
    out.plane_tb = A.plane_tb.data(); out.n_plane_tb = (uint32_t)A.plane_tb.size();
    out.order = A.order.data(); out.n_order = (uint32_t)A.order.size();
    return DG_OK;
}

namespace {
// Counting sort of records into FE_BIN_W-column strips, keeping their order (lo/hi: first / last column, inclusive).
template <typename T, typename Range>
void bin_by_columns(const std::vector<T> &recs, int W, Range range, std::vector<uint32_t> &off, std::vector<uint16_t> &idx) {
    const int nb = (W + FE_BIN_W - 1) / FE_BIN_W;
    off.assign((size_t)nb + 1, 0u);
    for (const T &r : recs) {
        int lo, hi;
        if (!range(r, lo, hi)) continue;
        for (int b = lo / FE_BIN_W; b <= hi / FE_BIN_W; b++) off[(size_t)b + 1]++;
    }
    for (int b = 0; b < nb; b++) off[(size_t)b + 1] += off[(size_t)b];
    idx.resize(off[(size_t)nb]);
    std::vector<uint32_t> cur(off.begin(), off.end() - 1);
    for (size_t i = 0; i < recs.size(); i++) {
        int lo, hi;
        if (!range(recs[i], lo, hi)) continue;
        for (int b = lo / FE_BIN_W; b <= hi / FE_BIN_W; b++) idx[cur[(size_t)b]++] = (uint16_t)i;
    }
}
}  // namespace

int build_frame_parts(const Scene &sc, int W, int H, const dg_view &view, FrameArena &A, std::string &err, const ViewInputs &in, const SceneFx *fx) {
    if (W <= 0 || H <= 0 || W > 16384 || H > 16384) { err = "bad frame size"; return DG_ERR_INVALID; }
    A.parts.clear(); A.sprites.clear(); A.behind.clear(); A.sky_parts.clear(); A.behind_words = 0; A.n_sky_slots = 0;
    A.recs->clear();
    Walker wk(sc, W, H, view, A, err, in, fx);
    if (wk.status) return wk.status;
    wk.parts_mode = true;
    wk.walk_bsp();
    if (wk.status) return wk.status;
    wk.map_objects();
    if (wk.status) return wk.status;
    if (A.sprites.size() > 65535) { err = "more than 65535 sprites in a frame"; return kPartsUnsupported; }
    bin_by_columns(A.parts, W, [](const FePart &p, int &lo, int &hi) { lo = p.sx; hi = p.ex; return true; }, A.bin_off, A.bin_parts);
    bin_by_columns(A.sprites, W, [](const FeSprite &s, int &lo, int &hi) { lo = s.x0; hi = s.x1 - 1; return s.x0 < s.x1; }, A.sbin_off, A.sbin_sprites);
    return DG_OK;
}

}  // namespace dg
