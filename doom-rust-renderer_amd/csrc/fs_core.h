// fs_core.h — the per-seg and per-sprite half of the reference's front end as host/device inline functions: what
// Segs::process_seg (src/renderer/segs.rs:353-590) and Segs::process_sidedef (:121-200) do BEFORE the column loop, clip_to_viewport and
// the projection (src/renderer/misc.rs:13-161, src/geometry.rs:56-86, src/map/vertexes.rs:20-34) and the per-object part of
// draw_map_objects (src/renderer/map_objects.rs:34-129).  Three callers execute these bodies:
//   * frontend.cpp  Walker (host, list mode): dg_build_lists, DG_FE_HOST, depth / labels / bundles, every frame a device front end hands
//     back.  It takes the geometry (fs_seg, fs_part_geom, fs_part_offsets, fs_mobj_geom) and runs its own column loops after it;
//   * frontend.cpp  Walker (host, parts mode): one thread per frame walks the BSP in order and records fs_part / fs_mobj (DG_FE_DEVICE);
//   * fs_kernels.hip (GPU, DG_FE_DEVICE_SEGS): one lane per (frame, seg) / (frame, map object), order restored afterwards —
// and tests/emul runs the GPU's bodies on the CPU against the host walker, record by record.
// Arithmetic contract as everywhere: IEEE f32 in the reference's operand order, no contraction, Rust `as` casts through rust_num.h.
#pragma once
#include "fe_dev.h"
#include "rust_num.h"

namespace dg {

struct V2 { float x, y; };
struct Seg2 { V2 a, b; };

DG_HD V2 v2_sub(V2 p, V2 q) { return V2{p.x - q.x, p.y - q.y}; }
DG_HD V2 v2_rot(V2 v, float c, float s) { return V2{v.x * c - v.y * s, v.y * c + v.x * s}; }      // vertexes.rs:20-25
DG_HD bool left_of(V2 v, const Seg2 &l) {                                                             // vertexes.rs:27-34
    V2 p = v2_sub(v, l.a), d = v2_sub(l.b, l.a);
    return p.x * d.y - p.y * d.x <= 0.0f;
}
DG_HD float v2_dist(V2 p, V2 q) { float dx = p.x - q.x, dy = p.y - q.y; return __builtin_sqrtf(dx * dx + dy * dy); }
DG_HD float fs_fmin(float a, float b) { return __builtin_fminf(a, b); }
DG_HD float fs_fmax(float a, float b) { return __builtin_fmaxf(a, b); }

// Line::intersection, src/geometry.rs:56-82
DG_HD bool line_intersect(const Seg2 &m, const Seg2 &n, V2 &out) {
    float x1 = m.a.x, y1 = m.a.y, x2 = m.b.x, y2 = m.b.y, x3 = n.a.x, y3 = n.a.y, x4 = n.b.x, y4 = n.b.y;
    float quot = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4);
    if (__builtin_fabsf(quot) < 0.001f) return false;
    float inv = 1.0f / quot;
    float c12 = x1 * y2 - y1 * x2, c34 = x3 * y4 - y3 * x4;
    out.x = inv * (c12 * (x3 - x4) - (x1 - x2) * c34);
    out.y = inv * (c12 * (y3 - y4) - (y1 - y2) * c34);
    return true;
}

struct Clipped { Seg2 line; float start_offset; };

// clip_to_viewport, src/renderer/misc.rs:13-115
DG_HD bool clip_to_viewport(const Seg2 &line, Clipped &out) {
    const Seg2 left{{0.0f, 0.0f}, {1.0f, 1.0f}}, right{{0.0f, 0.0f}, {1.0f, -1.0f}};
    bool s_out_l = left_of(line.a, left), e_out_l = left_of(line.b, left);
    bool s_out_r = !left_of(line.a, right), e_out_r = !left_of(line.b, right);
    bool s_in = line.a.x > 0.0f && !s_out_l && !s_out_r;
    bool e_in = line.b.x > 0.0f && !e_out_l && !e_out_r;
    if (s_in && e_in) { out.line = line; out.start_offset = 0.0f; return true; }
    V2 li{0.0f, 0.0f}, ri{0.0f, 0.0f};
    bool l_hit = line_intersect(line, left, li) && li.x >= 0.0f;
    bool r_hit = line_intersect(line, right, ri) && ri.x >= 0.0f;
    if (!s_in && !e_in && !l_hit && !r_hit) return false;
    if (!s_in && !e_in && (l_hit != r_hit)) return false;
    if ((r_hit && s_out_r && e_out_r) || (l_hit && s_out_l && e_out_l)) return false;
    V2 s = line.a, e = line.b;
    float so = 0.0f;
    if (l_hit) {
        if (s_out_l) { so = v2_dist(li, s); s = li; }
        if (e_out_l) e = li;
    }
    if (r_hit) {
        if (s_out_r) s = ri;
        if (e_out_r) e = ri;
    }
    out.line = Seg2{s, e};
    out.start_offset = so;
    return true;
}

struct ScreenLine { int32_t sx, sy, ex, ey; };

// perspective_transform + make_sidedef_non_vertical_line, src/renderer/misc.rs:130-161.  K: FrameConsts (host) or DevConsts (device).
template <typename K> DG_HD ScreenLine project(const K &k, const Seg2 &l, float height) {
    float tsx = k.GCFX * l.a.y / l.a.x, tsy = k.GCFX * height / l.a.x;
    float tex = k.GCFX * l.b.y / l.b.x, tey = k.GCFX * height / l.b.x;
    tsx *= k.ARC;
    tex *= k.ARC;
    ScreenLine o;
    o.sx = f32_as_i32(k.CFX - tsx);
    o.sy = f32_as_i32(k.CFY - tsy);
    o.ex = f32_as_i32(k.CFX - tex);
    o.ey = f32_as_i32(k.CFY - tey);
    o.sx = o.sx < k.W - 1 ? o.sx : k.W - 1;
    o.ex = o.ex < k.W - 1 ? o.ex : k.W - 1;
    return o;
}

// The slope of a projected edge, in rows per column (segs.rs:147-150, map_objects.rs:121-124)
DG_HD float fs_slope(const ScreenLine &l) { return ((float)l.sy - (float)l.ey) / ((float)l.sx - (float)l.ex); }

// BitmapRender::is_behind_vertex (bitmap_render.rs:137-165) for a record's clipped line; min_x / max_x: of its two ends (the host keeps them)
DG_HD bool fs_behind(const Seg2 &line, float min_x, float max_x, V2 v) {
    if (min_x > v.x) return true;
    if (max_x > v.x && !left_of(v, line)) return true;
    return false;
}
DG_HD bool fs_behind(const Seg2 &line, V2 v) { return fs_behind(line, fs_fmin(line.a.x, line.b.x), fs_fmax(line.a.x, line.b.x), v); }

// What the texture mapper needs of a bitmap (scene.hpp BitmapInfo; the GPU holds a table of these)
struct FsBitmap { uint32_t texel_off; int16_t w, h; int16_t top_offset; uint16_t has_holes; };
static_assert(sizeof(FsBitmap) == 12, "FsBitmap layout");

// Per-record constants of render_vertical_bitmap_line (bitmap_render.rs:233-251)
DG_HD DevWallRec fs_wall_rec(const FsBitmap &bi, float lsx, float lsy, float lex, float ley, float start_offset, int32_t start_x, int32_t end_x,
                             float bottom_height, float top_height, int16_t offset_x, int16_t offset_y, int16_t light_level) {
    DevWallRec d;
    float dx = lsx - lex, dy = lsy - ley;
    float len = __builtin_sqrtf(dx * dx + dy * dy);             // Line::length, geometry.rs:84-86
    float uz0 = lsx, uz1 = lex;
    d.A = 0.0f / uz0;
    d.B = len / uz1;
    d.C = 1.0f / uz0;
    d.D = 1.0f / uz1;
    d.uy1 = top_height - bottom_height;
    d.lightf = (float)light_level / 255.0f;
    d.dxf = (float)(end_x - start_x);
    d.start_x = start_x;
    d.texel_off = bi.texel_off;
    d.w = bi.w; d.h = bi.h;
    d.off_x = (int16_t)wrap_i16(f32_as_i16(start_offset) + offset_x);
    d.off_y = offset_y;
    d.has_holes = bi.has_holes;
    return d;
}

// ---- one seg -----------------------------------------------------------------------------------------------------------------------
// Everything process_seg reads about a seg, flattened once per scene (Scene::fs_segs; the same table is uploaded to the GPU).
struct FsSeg {
    float v1x, v1y, v2x, v2y;
    int32_t front_sector, back_sector;      // front_sector < 0: the seg's side has no sidedef (segs.rs:358-362: skipped); back_sector < 0: one-sided
    float sd_xoff, sd_yoff;                 // front sidedef offsets
    int32_t tex_mid, tex_low, tex_up;       // bitmap id, TEX_NONE (-1) for "-", TEX_UNKNOWN (-2) when Textures::get would panic
    int16_t seg_offset;
    uint16_t ld_flags;                      // linedef flags: 4 two-sided, 8 upper unpegged, 16 lower unpegged (linedefs.rs:10-18)
};
static_assert(sizeof(FsSeg) == 48, "FsSeg layout");
struct FsSector {                           // a sector as loaded (its light level is game state, and so are its two heights: a view may
    int16_t floor_h, ceil_h;                // bring its own through FsRowHeights below; these are the loaded ones)
    int32_t floor_flat, ceil_flat;          // flat id (>= 0) when not animated, FLAT_MISSING (-2) when the lump does not exist
    int32_t floor_anim, ceil_anim;          // index into the animation lists, or -1
    uint32_t ceil_tex_sky;                  // sector.ceiling_texture.contains("SKY") (segs.rs:463-469)
};
static_assert(sizeof(FsSector) == 24, "FsSector layout");
struct FsAnim { int32_t n; int32_t flat[4]; };

// Flats::get_animated at this frame's timestamp (flats.rs:103-111)
DG_HD int32_t fs_resolve_flat(int32_t flat, int32_t anim, const FsAnim *anims, float timestamp) {
    if (anim < 0) return flat;
    const FsAnim &a = anims[anim];
    float t = timestamp * 3.0f;
    unsigned long long cyc = !(t > 0.0f) ? 0ull : (t >= 18446744073709551616.0f ? ~0ull : (unsigned long long)t);
    return a.flat[cyc % (unsigned long long)a.n];
}

// ---- wall effects (dg_scene_set_wall_effects) ----------------------------------------------------------------------
// Per seg, what the scene's effect flags change about its sidedef: the scroll count k (linedefs of special 48 whose front sidedef it is;
// 0 without DG_WALL_SCROLL) and, per texture slot, the live animation list it belongs to (-1: static; always -1 without DG_WALL_ANIMATE).
// The lists are FsAnim records over bitmap ids.
struct FsSegFx { uint32_t scroll_k; int8_t anim_mid, anim_low, anim_up; uint8_t pad; };
static_assert(sizeof(FsSegFx) == 8, "FsSegFx layout");
// Clock::ticks: Rust's `(timestamp * 35.0f32) as u32` (saturating, NaN -> 0)
DG_HD uint32_t fs_tics(float timestamp) {
    const float t = timestamp * 35.0f;
    return !(t > 0.0f) ? 0u : (t >= 4294967296.0f ? 0xffffffffu : (uint32_t)t);
}
// The seg as its sidedef reads at `timestamp`: each animated texture is its list's frame (the flat rule, fs_resolve_flat), and the x
// offset is moved by k * tics mod 2^16 (vanilla's += FRACUNIT per tic and linedef, in whole texels).
DG_HD void fs_seg_fx(FsSeg &sg, const FsSegFx &fx, const FsAnim *lists, float timestamp) {
    sg.tex_mid = fs_resolve_flat(sg.tex_mid, fx.anim_mid, lists, timestamp);
    sg.tex_low = fs_resolve_flat(sg.tex_low, fx.anim_low, lists, timestamp);
    sg.tex_up = fs_resolve_flat(sg.tex_up, fx.anim_up, lists, timestamp);
    if (fx.scroll_k) {
        const uint32_t d = (fx.scroll_k * fs_tics(timestamp)) & 0xffffu;
        sg.sd_xoff = (float)wrap_i16(f32_as_i16(sg.sd_xoff) + (int32_t)d);
    }
}
// What fs_seg does to a seg's sidedef before it reads its textures and x offset: FsNoFx nothing (the seg itself — the default, and what
// every caller without effects compiles to), FsFx the scene's wall effects (a copy of the seg through fs_seg_fx).
struct FsNoFx {
    DG_HD const FsSeg &seg(const FsSeg &sg, uint32_t, float) const { return sg; }
};
struct FsFx {
    const FsSegFx *fx; const FsAnim *lists;      // per seg; the live animation lists
    DG_HD FsSeg seg(const FsSeg &sg, uint32_t si, float timestamp) const {
        FsSeg o = sg;
        fs_seg_fx(o, fx[si], lists, timestamp);
        return o;
    }
};

// Where fs_seg / fs_mobj read a sector's floor and ceiling heights (Sector.floor_height / .ceiling_height, game state in the reference:
// segs.rs:376-402,463-484, map_objects.rs:115).  FsOwnHeights: the scene table's own fields, the heights as loaded — the default, and what
// every caller without per-view heights compiles to.  FsRowHeights: the view's row [sector] (dg_view_sectors, view_rows_core.h).
// Both take the sector's record and its index, and hand back one height: stated so, the default reads exactly the field the caller
// read before there was a policy.
struct alignas(4) FsHeights { int16_t floor_h, ceil_h; };
static_assert(sizeof(FsHeights) == 4, "FsHeights layout");
struct FsOwnHeights {
    DG_HD int16_t floor(const FsSector &s, int32_t) const { return s.floor_h; }
    DG_HD int16_t ceil(const FsSector &s, int32_t) const { return s.ceil_h; }
};
struct FsRowHeights {
    const FsHeights *row;                        // [n_sectors] of the frame
    DG_HD int16_t floor(const FsSector &, int32_t i) const { return row[i].floor_h; }
    DG_HD int16_t ceil(const FsSector &, int32_t i) const { return row[i].ceil_h; }
};
// The heights policy an effects policy carries: none (FsOwnHeights) unless it is an FsWithRows.
template <typename Fx> struct FsWithRows : Fx { FsRowHeights ht; };
template <typename Fx> DG_HD FsOwnHeights fs_heights_of(const Fx &) { return FsOwnHeights(); }
template <typename Fx> DG_HD FsRowHeights fs_heights_of(const FsWithRows<Fx> &x) { return x.ht; }

// ---- per-view surfaces (dg_view_surfaces) ------------------------------------------------------------------------------
// A sector's two flats as one view has them, 8 bytes: each word is a flat handle — the flat id, or FS_FLAT_ANIM | the animation list
// (Flats::get_animated goes by the name's list, whichever member the name is), FS_FLAT_MISSING when the lump does not exist, and
// FS_FLAT_SKY when the name contains "SKY" (what the sky hack asks of the ceiling's, segs.rs:463-469).  Never negative.
enum : int32_t { FS_FLAT_INDEX = 0x0fffffff, FS_FLAT_MISSING = 1 << 28, FS_FLAT_SKY = 1 << 29, FS_FLAT_ANIM = 1 << 30 };
struct alignas(8) FsFlats { int32_t floor, ceil; };
static_assert(sizeof(FsFlats) == 8, "FsFlats layout");
DG_HD int32_t fs_flat_handle(int32_t flat, int32_t anim, bool sky) {
    return (anim >= 0 ? FS_FLAT_ANIM | anim : flat >= 0 ? flat : FS_FLAT_MISSING) | (sky ? FS_FLAT_SKY : 0);
}
DG_HD int32_t fs_handle_flat(int32_t h) { return h & (FS_FLAT_ANIM | FS_FLAT_MISSING) ? (h & FS_FLAT_MISSING ? -2 : 0) : h & FS_FLAT_INDEX; }   // (-2: FLAT_MISSING)
DG_HD int32_t fs_handle_anim(int32_t h) { return h & FS_FLAT_ANIM ? h & FS_FLAT_INDEX : -1; }

// One sidedef as one view has it, 24 bytes: the three bitmap ids (TEX_NONE for "-"), the live wall animation list of each (-1: none, and
// always -1 without DG_WALL_ANIMATE) and the two offsets.  A frame's entries are sorted by sidedef and unique (resolve_view_surfaces).
struct FsSideEntry { int32_t sidedef; int32_t tex_mid, tex_low, tex_up; int8_t anim_mid, anim_low, anim_up, pad; int16_t x_offset, y_offset; };
static_assert(sizeof(FsSideEntry) == 24, "FsSideEntry layout");
// The entry of `sidedef` among the n sorted entries at e, or -1: a binary search, at most ceil(log2(n + 1)) probes of 4 bytes.
DG_HD int32_t fs_side_find(const FsSideEntry *e, uint32_t n, int32_t sidedef) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (e[mid].sidedef < sidedef) lo = mid + 1; else hi = mid;
    }
    return lo < n && e[lo].sidedef == sidedef ? (int32_t)lo : -1;
}
// The seg with an entry's sidedef in place of its own, and what the wall effects then make of it: the scroll count stays the sidedef's
// (special 48 belongs to the linedef), the animation lists are those of the entry's textures.
DG_HD void fs_side_fx(const FsNoFx &, FsSeg &, uint32_t, const FsSideEntry &, float) {}
DG_HD void fs_side_fx(const FsFx &fx, FsSeg &o, uint32_t si, const FsSideEntry &en, float timestamp) {
    fs_seg_fx(o, FsSegFx{fx.fx[si].scroll_k, en.anim_mid, en.anim_low, en.anim_up, 0}, fx.lists, timestamp);
}
// Where fs_seg reads a sidedef's textures and offsets and a sector's flats (game state in the reference: segs.rs:121-200,450-469,
// 493-588), asked per field.  FsOwnSurfaces: the seg's and the scene table's own fields, as loaded — the default, and the loads every
// caller without per-view surfaces made before there was a policy.  FsViewSurfaces: the view's row [sector] of flats and its sorted
// span of sidedef entries, searched by the seg's front sidedef (seg_side[seg]).
struct FsOwnSurfaces {
    template <typename Fx> DG_HD decltype(auto) seg(const Fx &fx, const FsSeg &sg, uint32_t si, float timestamp) const { return fx.seg(sg, si, timestamp); }
    DG_HD int32_t floor_flat(const FsSector &s, int32_t) const { return s.floor_flat; }
    DG_HD int32_t floor_anim(const FsSector &s, int32_t) const { return s.floor_anim; }
    DG_HD int32_t ceil_flat(const FsSector &s, int32_t) const { return s.ceil_flat; }
    DG_HD int32_t ceil_anim(const FsSector &s, int32_t) const { return s.ceil_anim; }
    DG_HD bool ceil_sky(const FsSector &s, int32_t) const { return s.ceil_tex_sky != 0; }
};
struct FsViewSurfaces {
    const FsFlats *row;                          // [n_sectors] of the frame
    const FsSideEntry *sides; uint32_t n_sides;  // the frame's span
    const int32_t *seg_side;                     // [n_segs] front sidedef of every seg (-1: none)
    template <typename Fx> DG_HD FsSeg seg(const Fx &fx, const FsSeg &sg, uint32_t si, float timestamp) const {
        const int32_t at = n_sides ? fs_side_find(sides, n_sides, seg_side[si]) : -1;
        if (at < 0) return fx.seg(sg, si, timestamp);
        const FsSideEntry en = sides[at];
        FsSeg o = sg;
        o.tex_mid = en.tex_mid; o.tex_low = en.tex_low; o.tex_up = en.tex_up;
        o.sd_xoff = (float)en.x_offset; o.sd_yoff = (float)en.y_offset;
        fs_side_fx(fx, o, si, en, timestamp);
        return o;
    }
    DG_HD int32_t floor_flat(const FsSector &, int32_t i) const { return fs_handle_flat(row[i].floor); }
    DG_HD int32_t floor_anim(const FsSector &, int32_t i) const { return fs_handle_anim(row[i].floor); }
    DG_HD int32_t ceil_flat(const FsSector &, int32_t i) const { return fs_handle_flat(row[i].ceil); }
    DG_HD int32_t ceil_anim(const FsSector &, int32_t i) const { return fs_handle_anim(row[i].ceil); }
    DG_HD bool ceil_sky(const FsSector &, int32_t i) const { return (row[i].ceil & FS_FLAT_SKY) != 0; }
};
// The surfaces policy an effects policy carries: none (FsOwnSurfaces) unless it is an FsWithSurfaces, which has height rows too.
template <typename Fx> struct FsWithSurfaces : FsWithRows<Fx> { FsViewSurfaces sf; };
template <typename Fx> DG_HD FsOwnSurfaces fs_surfaces_of(const Fx &) { return FsOwnSurfaces(); }
template <typename Fx> DG_HD FsViewSurfaces fs_surfaces_of(const FsWithSurfaces<Fx> &x) { return x.sf; }
template <typename Fx> DG_HD FsRowHeights fs_heights_of(const FsWithSurfaces<Fx> &x) { return x.ht; }

enum : int32_t {                             // outcome of fs_seg / fs_part
    FS_OK = 0,
    FS_SKIP = 1,                             // nothing to record (not an error)
    FS_FAIL_CLIP_X = 2,                      // "Clipped line x < -0.01" (segs.rs:431-436)
    FS_FAIL_FLAT = 3,                        // Flat::new unwrap (flats.rs:117)
    FS_FAIL_TEXTURE = 4,                     // Textures::get panics (textures.rs:158)
    FS_FAIL_VERTICAL = 5,                    // "Wall start not vertical" (segs.rs:140-145)
    FS_FAIL_LINE_X = 6,                      // "Invalid line x" (segs.rs:103-111)
    FS_FAIL_PARTS = 7,                       // only the host list path can judge (zero-sized bitmap)
};

struct FsCall {                              // one process_sidedef call of a seg (segs.rs:493-588)
    float bottom_height, top_height;
    int32_t offset_y, tex;
    uint32_t flags;                          // FEP_ONLY_OCCL | FEP_LOWER | FEP_UPPER | FEP_DRAW_CEILING | FEP_TWO_SIDED_MID
};
struct FsSegOut {                            // process_seg up to its process_sidedef calls
    Clipped cl;
    int16_t seg_offset, floor_h, ceil_h, light;
    int32_t floor_flat, ceil_flat;
    float sd_xoff, sd_yoff;
    int32_t n_calls;                         // slots to look at: 1 (one-sided) or 4; call_mask says which of them hold a call.  The slots
    uint32_t call_mask;                      // are fixed — only-occlusion, two-sided middle, lower, upper (the reference's order) — so that
    FsCall call[4];                          // every index into call[] is a constant (an indexed array would live in scratch memory on the GPU)
};
// The call in slot i (a constant after unrolling).
DG_HD FsCall fs_call(const FsSegOut &o, uint32_t i) { return i == 0u ? o.call[0] : i == 1u ? o.call[1] : i == 2u ? o.call[2] : o.call[3]; }

// Segs::process_seg, segs.rs:353-590, for a viewer at ppos looking along (cos_na, sin_na) = (cos, sin)(-angle).  light: the front
// sector's CURRENT light level.  Returns FS_OK with 1 .. 5 calls, FS_SKIP, or a failure.  fx / si: the wall effects and the seg's index
// (applied past the clip and back-face tests, so that the segs turned away there never look at them); sf: the surfaces policy, asked there too.
template <typename K, typename Fx = FsNoFx, typename Ht = FsOwnHeights, typename Sf = FsOwnSurfaces>
DG_HD int32_t fs_seg(const K &k, const FsSeg &sg, const FsSector *sectors, const FsAnim *anims, V2 ppos, float cos_na, float sin_na, float player_height,
                     float timestamp, int16_t light, FsSegOut &o, const Fx &fx = Fx(), uint32_t si = 0, const Ht &ht = Ht(), const Sf &sf = Sf()) {
    if (sg.front_sector < 0) return FS_SKIP;
    // (the clip comes first here: it needs the seg's two vertices only and turns away most segs of a map; the sector heights the
    // reference reads before it — segs.rs:364-402 — have no side effects and are read below, by the segs that are left)
    V2 a = v2_rot(v2_sub(V2{sg.v1x, sg.v1y}, ppos), cos_na, sin_na);
    V2 b = v2_rot(v2_sub(V2{sg.v2x, sg.v2y}, ppos), cos_na, sin_na);
    if (!clip_to_viewport(Seg2{a, b}, o.cl)) return FS_SKIP;
    if (o.cl.line.a.x < -0.01f) return FS_FAIL_CLIP_X;

    const FsSector &fs = sectors[sg.front_sector];
    const FsSector *bs = sg.back_sector >= 0 ? &sectors[sg.back_sector] : nullptr;
    const int16_t fs_floor_h = ht.floor(fs, sg.front_sector), fs_ceil_h = ht.ceil(fs, sg.front_sector);
    float floor_height = (float)fs_floor_h, ceiling_height = (float)fs_ceil_h;
    bool has_pb = false, has_pt = false;
    float pb_h = 0.0f, pt_h = 0.0f;
    if (bs) {
        if (ht.floor(*bs, sg.back_sector) > fs_floor_h) { has_pb = true; pb_h = (float)ht.floor(*bs, sg.back_sector); }
        if (ht.ceil(*bs, sg.back_sector) < fs_ceil_h) { has_pt = true; pt_h = (float)ht.ceil(*bs, sg.back_sector); }
    }
    const bool two_sided = (sg.ld_flags & 4) != 0, top_unpegged = (sg.ld_flags & 8) != 0, bottom_unpegged = (sg.ld_flags & 16) != 0;

    ScreenLine fl = project(k, o.cl.line, floor_height - player_height);
    if (fl.sx > fl.ex) return FS_SKIP;                            // back face
    const auto &sw = sf.seg(fx, sg, si, timestamp);               // the sidedef's textures and offsets as drawn at this timestamp

    o.floor_flat = fs_resolve_flat(sf.floor_flat(fs, sg.front_sector), sf.floor_anim(fs, sg.front_sector), anims, timestamp);
    o.ceil_flat = fs_resolve_flat(sf.ceil_flat(fs, sg.front_sector), sf.ceil_anim(fs, sg.front_sector), anims, timestamp);
    if (o.floor_flat < 0 || o.ceil_flat < 0) return FS_FAIL_FLAT;

    bool draw_ceiling = true;
    if (bs && sf.ceil_sky(fs, sg.front_sector) && sf.ceil_sky(*bs, sg.back_sector)) {              // sky hack, segs.rs:463-477
        has_pt = false;
        ceiling_height = fs_fmin((float)ht.ceil(*bs, sg.back_sector), ceiling_height);
        draw_ceiling = false;
    }
    o.seg_offset = sg.seg_offset; o.floor_h = fs_floor_h; o.ceil_h = fs_ceil_h; o.light = light;
    o.sd_xoff = sw.sd_xoff; o.sd_yoff = sw.sd_yoff;
    const uint32_t dc = draw_ceiling ? FEP_DRAW_CEILING : 0u;
    if (!two_sided) {
        const int32_t oy = bottom_unpegged ? f32_as_i32(floor_height - ceiling_height) : 0;
        o.call[0] = FsCall{floor_height - player_height, ceiling_height - player_height, oy, sw.tex_mid, dc};
        o.n_calls = 1; o.call_mask = 1u;
        return FS_OK;
    }
    o.call[0] = FsCall{floor_height - player_height, ceiling_height - player_height, 0, sw.tex_mid, dc | FEP_ONLY_OCCL};
    const float mid_floor = has_pb ? pb_h : floor_height, mid_ceil = has_pt ? pt_h : ceiling_height;
    o.call[1] = FsCall{mid_floor - player_height, mid_ceil - player_height, 0, sw.tex_mid, dc | FEP_TWO_SIDED_MID};
    o.call_mask = 3u;
    if (has_pb) {
        const int32_t oy = bottom_unpegged ? f32_as_i32(ceiling_height - pb_h) : 0;
        o.call[2] = FsCall{floor_height - player_height, pb_h - player_height, oy, sw.tex_low, dc | FEP_LOWER};
        o.call_mask |= 4u;
    }
    if (has_pt) {
        const int32_t oy = top_unpegged ? 0 : f32_as_i32(pt_h - ceiling_height);
        o.call[3] = FsCall{pt_h - player_height, ceiling_height - player_height, oy, sw.tex_up, dc | FEP_UPPER};
        o.call_mask |= 8u;
    }
    o.n_calls = 4;
    return FS_OK;
}

// The x half of make_sidedef_non_vertical_line (misc.rs:138-161): the screen columns of a clipped line do not depend on the height.
template <typename K> DG_HD void project_x(const K &k, const Seg2 &l, int32_t &sx, int32_t &ex) {
    float tsx = k.GCFX * l.a.y / l.a.x;
    float tex = k.GCFX * l.b.y / l.b.x;
    tsx *= k.ARC;
    tex *= k.ARC;
    sx = f32_as_i32(k.CFX - tsx);
    ex = f32_as_i32(k.CFX - tex);
    sx = sx < k.W - 1 ? sx : k.W - 1;
    ex = ex < k.W - 1 ? ex : k.W - 1;
}
// A part's FEP_* flags: the call's own, whether it draws a bitmap, and whether its sector's flats are sky.  flat_sky[flat]: the name contains "SKY".
DG_HD uint32_t fs_part_flags(const FsSegOut &s, const FsCall &c, const uint8_t *flat_sky) {
    const bool fsky = flat_sky[s.floor_flat] != 0, csky = flat_sky[s.ceil_flat] != 0;
    return c.flags | (c.tex >= 0 ? FEP_HAS_BITMAP : 0u) | (fsky ? FEP_FLOOR_SKY : 0u) | (csky ? FEP_CEIL_SKY : 0u);
}
// The texture offsets a part is drawn with: the sidedef's plus the seg's in x, the sidedef's plus the call's pegging offset in y (segs.rs:158-175)
DG_HD void fs_part_offsets(const FsSegOut &s, const FsCall &c, int16_t &offset_x, int16_t &offset_y) {
    offset_x = (int16_t)wrap_i16(f32_as_i16(s.sd_xoff) + s.seg_offset);
    offset_y = (int16_t)wrap_i16(f32_as_i16(s.sd_yoff) + wrap_i16(c.offset_y));
}
// The tests of Segs::process_sidedef (segs.rs:121-157) that decide whether a call reaches its column loop, and what the hidden-part
// culling needs of it: columns [sx, ex] and the FEP_* flags.  (Both edges of a part project to the same columns — the x of
// perspective_transform does not see the height — so the reference's "Wall start not vertical" panic cannot fire; fs_part keeps the test.)
template <typename K>
DG_HD int32_t fs_part_head(const K &k, const FsSegOut &s, const FsCall &c, const FsBitmap *bitmaps, const uint8_t *flat_sky, int32_t &sx, int32_t &ex, uint32_t &flags) {
    project_x(k, s.cl.line, sx, ex);
    if (c.tex == -2) return FS_FAIL_TEXTURE;                      // TEX_UNKNOWN
    if (wrap_i16(sx) == wrap_i16(ex)) return FS_SKIP;
    if (sx < 0 || sx >= k.W || ex < 0 || ex >= k.W) return FS_FAIL_LINE_X;
    if (c.tex >= 0 && (bitmaps[c.tex].w <= 0 || bitmaps[c.tex].h <= 0)) return FS_FAIL_PARTS;
    flags = fs_part_flags(s, c, flat_sky);
    return FS_OK;
}

// Segs::process_sidedef (segs.rs:121-200) up to its column loop, for one call of a seg: the FePart the device column walk consumes,
// without the two fields that depend on what came before in BSP order (sky_slot, seq: left -1 / 0).  FS_SKIP: a zero-width part.
// view_floor_height: player.floor_height (visplanes.rs:112).  flat_sky[flat]: the flat's name contains "SKY".
// The body is stated once for two callers: kGeomOnly stops in front of the FS_FAIL_PARTS test with the geometry in g (fs_part_geom: the
// host's list mode, which carries on with a zero-sized bitmap and reads none of the record); otherwise it fills p (fs_part).
struct FsPartGeom { ScreenLine bot, top; float bottom_delta, top_delta; };
template <bool kGeomOnly, typename K>
DG_HD int32_t fs_part_body(const K &k, const FsSegOut &s, const FsCall &c, const FsBitmap *bitmaps, const uint8_t *flat_sky, float view_floor_height, FsPartGeom *g,
                           FePart *pp) {
    const Seg2 &line = s.cl.line;
    const ScreenLine bot = project(k, line, c.bottom_height);
    const ScreenLine top = project(k, line, c.top_height);
    if (c.tex == -2) return FS_FAIL_TEXTURE;                      // TEX_UNKNOWN
    if (bot.sx != top.sx || bot.ex != top.ex) return FS_FAIL_VERTICAL;
    if (wrap_i16(bot.sx) == wrap_i16(bot.ex) || wrap_i16(top.sx) == wrap_i16(top.ex)) return FS_SKIP;
    if (bot.sx < 0 || bot.sx >= k.W || bot.ex < 0 || bot.ex >= k.W) return FS_FAIL_LINE_X;
    const float bottom_delta = fs_slope(bot), top_delta = fs_slope(top);
    if constexpr (kGeomOnly) { *g = FsPartGeom{bot, top, bottom_delta, top_delta}; return FS_OK; }
    FePart &p = *pp;
    if (c.tex >= 0 && (bitmaps[c.tex].w <= 0 || bitmaps[c.tex].h <= 0)) return FS_FAIL_PARTS;
    int16_t offset_x, offset_y;
    fs_part_offsets(s, c, offset_x, offset_y);
    p.sx = bot.sx; p.ex = bot.ex;
    p.bsy = (float)bot.sy; p.bsx = (float)bot.sx; p.bdelta = bottom_delta;
    p.tsy = (float)top.sy; p.tsx = (float)top.sx; p.tdelta = top_delta;
    p.flags = fs_part_flags(s, c, flat_sky);
    p.sky_slot = -1;
    p.seq = 0;
    p.pad = 0;
    if (c.tex >= 0) {
        p.wall = fs_wall_rec(bitmaps[c.tex], line.a.x, line.a.y, line.b.x, line.b.y, s.cl.start_offset, bot.sx, bot.ex, c.bottom_height, c.top_height,
                             offset_x, offset_y, s.light);
    } else {
        p.wall = DevWallRec{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0u, 0, 0, 0, 0, 0u};
    }
    const float lightf = (float)s.light / 255.0f;
    p.floor_plane.wz = (float)s.floor_h - view_floor_height - 41.0f;      // visplanes.rs:112
    p.floor_plane.gwz = k.GCFX * p.floor_plane.wz;
    p.floor_plane.lightf = lightf;
    p.floor_plane.flat_off = (uint32_t)s.floor_flat * 4096u;
    p.ceil_plane.wz = (float)s.ceil_h - view_floor_height - 41.0f;
    p.ceil_plane.gwz = k.GCFX * p.ceil_plane.wz;
    p.ceil_plane.lightf = lightf;
    p.ceil_plane.flat_off = (uint32_t)s.ceil_flat * 4096u;
    return FS_OK;
}
template <typename K>
DG_HD int32_t fs_part(const K &k, const FsSegOut &s, const FsCall &c, const FsBitmap *bitmaps, const uint8_t *flat_sky, float view_floor_height, FePart &p) {
    return fs_part_body<false>(k, s, c, bitmaps, flat_sky, view_floor_height, nullptr, &p);
}
template <typename K> DG_HD int32_t fs_part_geom(const K &k, const FsSegOut &s, const FsCall &c, FsPartGeom &g) {
    return fs_part_body<true>(k, s, c, nullptr, nullptr, 0.0f, &g, nullptr);
}
// Does a part with these flags open / extend visplanes (segs.rs:263-318), and may it therefore need a sky event slot?
DG_HD bool fs_part_wants_sky_slot(uint32_t flags) {
    const bool full_height = !(flags & (FEP_LOWER | FEP_UPPER | FEP_ONLY_OCCL));
    const bool planes_here = !(flags & FEP_TWO_SIDED_MID) && (full_height || (flags & FEP_ONLY_OCCL));
    return planes_here && ((flags & FEP_FLOOR_SKY) || ((flags & FEP_CEIL_SKY) && (flags & FEP_DRAW_CEILING)));
}
// A full-height solid part: every column it spans becomes horizontally occluded (segs.rs:341-344)
DG_HD bool fs_part_is_solid(uint32_t flags) { return !(flags & (FEP_LOWER | FEP_UPPER | FEP_ONLY_OCCL | FEP_TWO_SIDED_MID)); }

// ---- one map object ----------------------------------------------------------------------------------------------------------------
struct FsMobj { float x, y, angle; int32_t sector; };            // where the object is: as loaded, or a view's pose (mobj_pose_core.h); sector < 0: outside the map
static_assert(sizeof(FsMobj) == 16, "FsMobj layout");
struct FsSpriteFrame { int32_t rotate; int32_t bitmap[8]; };     // sprites.rs:20-23

enum : int32_t { FS_FAIL_ROTATION = 8, FS_FAIL_MOBJ_CLIP_X = 9, FS_FAIL_MOBJ_COLUMN = 10 };

struct FsSpriteOut { FeSprite sp; Seg2 line; V2 centre; int32_t sort_key; };
// draw_map_objects (map_objects.rs:34-129, 168-209) for one object whose state shows (sprite_frame >= 0): FS_OK with the FeSprite
// (seq / behind_off left 0), FS_SKIP, or a failure.  light: the object's sector's current light level.
// The body is stated once for two callers, like fs_part_body: kGeomOnly stops in front of the FS_FAIL_PARTS test with the geometry in g
// (fs_mobj_geom: the host's list mode; vpv is the object in view space, what is_behind_vertex is asked about); otherwise it fills o (fs_mobj).
struct FsMobjGeom {
    int32_t bitmap;
    Clipped cl;
    V2 vpv;
    float bottom_height, top_height;
    ScreenLine bot, top;
    int32_t x0, x1;                                               // columns [x0, x1)
    int16_t light, sort_key;
};
template <bool kGeomOnly, typename K, typename Ht>
DG_HD int32_t fs_mobj_body(const K &k, const FsMobj &m, const FsSpriteFrame &sf, const FsBitmap *bitmaps, const FsSector *sectors, V2 ppos, float view_angle,
                           float cos_na, float sin_na, float player_height, int32_t full_bright, int16_t sector_light, FsMobjGeom *g, FsSpriteOut *out, const Ht &ht) {
    const float kPi = 3.14159265358979323846f;
    float angle = view_angle - m.angle - kPi;
    angle += kPi / 16.0f;
    angle = __builtin_fmodf(angle, 2.0f * kPi);
    if (angle < 0.0f) angle += 2.0f * kPi;
    angle = __builtin_fmodf(angle, 2.0f * kPi);
    const int rotation = f32_as_u8(angle * 8.0f / (2.0f * kPi));
    if (rotation > 7) return FS_FAIL_ROTATION;
    const int bitmap = sf.rotate ? sf.bitmap[rotation] : sf.bitmap[0];
    const FsBitmap &bi = bitmaps[bitmap];

    const V2 vpv = v2_rot(v2_sub(V2{m.x, m.y}, ppos), cos_na, sin_na);
    const int16_t width = bi.w;
    const V2 a = v2_sub(vpv, V2{0.0f, (float)(int16_t)(-width) / 2.0f});
    const V2 b = v2_sub(vpv, V2{0.0f, (float)width / 2.0f});
    Clipped cl;
    if (!clip_to_viewport(Seg2{a, b}, cl)) return FS_SKIP;
    if (cl.line.a.x < -0.01f) return FS_FAIL_MOBJ_CLIP_X;
    if (m.sector < 0) return FS_SKIP;                             // "Thing is outside map"
    const FsSector &sec = sectors[m.sector];
    const int16_t sec_floor_h = ht.floor(sec, m.sector);
    const int16_t light = full_bright ? (int16_t)255 : sector_light;

    const int16_t bh = bi.h;
    float bottom_height = (float)sec_floor_h - player_height;
    float top_height = (float)sec_floor_h + (float)bh - 1.0f - player_height;
    bottom_height += (float)bi.top_offset - (float)bh;
    top_height += (float)bi.top_offset - (float)bh;
    const ScreenLine bot = project(k, cl.line, bottom_height);
    const ScreenLine top = project(k, cl.line, top_height);
    const int x0 = wrap_i16(bot.sx), x1 = wrap_i16(bot.ex);       // columns [x0, x1)
    if (x0 < x1 && (x0 < 0 || x1 > k.W)) return FS_FAIL_MOBJ_COLUMN;
    if constexpr (kGeomOnly) {
        *g = FsMobjGeom{bitmap, cl, vpv, bottom_height, top_height, bot, top, x0, x1, light, (int16_t)f32_as_i16(cl.line.a.x)};   // sort key: bitmap_render.rs:168-174
        return FS_OK;
    }
    if (bi.w <= 0 || bi.h <= 0) return FS_FAIL_PARTS;
    FsSpriteOut &o = *out;
    FeSprite &sp = o.sp;
    sp.x0 = x0; sp.x1 = x1;
    sp.bsy = (float)bot.sy; sp.bsx = (float)bot.sx; sp.bdelta = fs_slope(bot);
    sp.tsy = (float)top.sy; sp.tsx = (float)top.sx; sp.tdelta = fs_slope(top);
    sp.seq = 0; sp.behind_off = 0; sp.pad[0] = sp.pad[1] = 0;
    sp.wall = fs_wall_rec(bi, cl.line.a.x, cl.line.a.y, cl.line.b.x, cl.line.b.y, cl.start_offset, bot.sx, bot.ex, bottom_height, top_height, 0, 0, light);
    o.line = cl.line;
    o.centre = vpv;
    o.sort_key = f32_as_i16(cl.line.a.x);                         // bitmap_render.rs:168-174
    return FS_OK;
}

template <typename K, typename Ht = FsOwnHeights>
DG_HD int32_t fs_mobj(const K &k, const FsMobj &m, const FsSpriteFrame &sf, const FsBitmap *bitmaps, const FsSector *sectors, V2 ppos, float view_angle,
                      float cos_na, float sin_na, float player_height, int32_t full_bright, int16_t sector_light, FsSpriteOut &o, const Ht &ht = Ht()) {
    return fs_mobj_body<false>(k, m, sf, bitmaps, sectors, ppos, view_angle, cos_na, sin_na, player_height, full_bright, sector_light, nullptr, &o, ht);
}
template <typename K, typename Ht = FsOwnHeights>
DG_HD int32_t fs_mobj_geom(const K &k, const FsMobj &m, const FsSpriteFrame &sf, const FsBitmap *bitmaps, const FsSector *sectors, V2 ppos, float view_angle,
                           float cos_na, float sin_na, float player_height, int32_t full_bright, int16_t sector_light, FsMobjGeom &g, const Ht &ht = Ht()) {
    return fs_mobj_body<true>(k, m, sf, bitmaps, sectors, ppos, view_angle, cos_na, sin_na, player_height, full_bright, sector_light, &g, nullptr, ht);
}

}  // namespace dg
