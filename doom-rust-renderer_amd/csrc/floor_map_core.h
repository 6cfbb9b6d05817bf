// floor_map_core.h — the rule of the floor-textured player-centred map frames as host/device inline functions:
// which map point a pixel's centre is, which subsector lies under it, whether the point is inside that subsector, and what the sector's
// floor looks like there.  floor_map_kernels.hip runs them on the GPU, floor_map_host.hpp on the host (dg_floor_map_host), and
// tests/floor_map/floor_map_host_main.cpp runs the kernel's phases as a host loop over the same functions against the literal rule.
//
// The lines and the arrow are ego_core.h's, unchanged: a pixel on which dg_ego_map_host draws has exactly that colour.  Every other pixel
// (X, Y), every operation in f32 in this order, no contraction (the units are built with -ffp-contract=off), no division (the host
// passes inv = 1.0f / scale):
//     r = ((float)(X - W / 2) + 0.5f) * inv,  f = ((float)(H / 2 - Y) - 0.5f) * inv          the inverse of ego_point_f at the pixel centre
//     rotate:  dx = r * sin_a + f * cos_a,  dy = f * sin_a - r * cos_a        else  dx = r, dy = f
//     mx = view.x + dx,  my = view.y + dy
//     leaf    from the root by walk_left_of, as pose_sector_at descends; its sector (walk_leaf_sector) -1: background
//     inside  for every seg v1 -> v2 of the leaf in lump order: (mx - v1x) * (v2y - v1y) - (my - v1y) * (v2x - v1x) < 0.0f: background
//             (the BSP gives every point of the plane a leaf, solid rock and the outside included: strictly behind a seg is not the subsector)
//     floor   the frame's cell of the sector (floor_cell): its flat at the view's timestamp, -1 for a missing flat or a sky floor
//             (background), and light_factor(light / 255, 0) of the light the colour frame of the view would use
//     texel   tx = (i32) floorf(mx) & 63, ty = (i32) floorf(my) & 63, flat[ty][tx] (both axes positive, visplanes.rs:119-125), the colour
//             shade(palette[texel], factor) — diminish_color at distance 0.
// Background is (0, 0, 0).  With a mask a sector is shown only if its bit is set in the frame's sector row (floor_seen_line: a linedef
// whose bit is set in the mask shows the sectors of both its sidedefs).
// In contract (ego_check_call / ego_check_view: W, H <= 16384, scale >= 2^-10, |view.x|, |view.y| <= 65536, |cos_a|, |sin_a| <= 1)
// |r|, |f| <= 8192.5 * 1024 < 2^23.01, |dx|, |dy| <= 2 * 2^23.01 and |mx|, |my| <= 65536 + 2^24.01 — so the bound the texel step needs
// is stated on its own: |mx|, |my| < 2^24 holds whenever scale >= 2^-9 or the frame is at most 8192 wide and high, and floor_texel
// itself is defined for every finite value: beyond +-2^31 the conversion saturates on both sides alike (rust_num.h's f32_as_i32).
#pragma once
#include <cmath>

#include "ego_core.h"
#include "fs_core.h"
#include "raster_core.h"
#include "walk_core.h"

namespace dg {

constexpr uint32_t FLOOR_VALUE = 0x80000000u;             // owner-tile word of a floor pixel: this bit | its RGB24 (a line's value lies below it)

struct FloorLeaf { uint32_t first, count; int32_t sector; };      // a subsector's segs in the seg table, and walk_leaf_sector
static_assert(sizeof(FloorLeaf) == 12, "FloorLeaf");
struct FloorSeg { float v1x, v1y, v2x, v2y; };
static_assert(sizeof(FloorSeg) == 16, "FloorSeg");
struct FloorLine { int32_t front, back; };                // the sectors a linedef's two sidedefs face (-1: no sidedef)
static_assert(sizeof(FloorLine) == 8, "FloorLine");
struct alignas(8) FloorCell { int32_t flat; float factor; };      // [frame][sector]: flat id (-1: background) and the shade factor
static_assert(sizeof(FloorCell) == 8, "FloorCell");

// The scene's tables as the descent reads them (device or host memory).  root = n_nodes - 1; no nodes: the one leaf 0.
struct FloorTables {
    const WalkNode *nodes; uint32_t n_nodes;
    const FloorLeaf *leaves; uint32_t n_leaves;
    const FloorSeg *segs; uint32_t n_segs;
    const uint8_t *flats; uint32_t n_flats;               // the flat pool, 4096 bytes each, [y][x]
    const uint32_t *palette;                              // 256 x r | g << 8 | b << 16
    uint32_t n_sectors;
};

// Step 1: the map point of pixel (X, Y)'s centre.
DG_HD void floor_map_point(int32_t X, int32_t Y, int32_t W, int32_t H, const EgoView &v, float inv, bool rotate, float &mx, float &my) {
    const float r = ((float)(X - W / 2) + 0.5f) * inv;
    const float f = ((float)(H / 2 - Y) - 0.5f) * inv;
    float dx = r, dy = f;
    if (rotate) {
        dx = r * v.sin_a + f * v.cos_a;
        dy = f * v.sin_a - r * v.cos_a;
    }
    mx = v.x + dx;
    my = v.y + dy;
}

// Step 2: the leaf under (mx, my), or -1 when an index read from the tables is out of range (never, for tables built by floor_tables).
DG_HD int32_t floor_leaf_at(const FloorTables &t, float mx, float my) {
    int32_t c = (int32_t)t.n_nodes - 1;
    while (c >= 0) {
        if ((uint32_t)c >= t.n_nodes) return -1;
        c = t.nodes[c].child[walk_left_of(t.nodes[c], mx, my) ? 1 : 0];
    }
    return (uint32_t)~c < t.n_leaves ? ~c : -1;
}

// Step 3 for one seg: is the point strictly behind it?
DG_HD bool floor_behind(const FloorSeg &s, float mx, float my) {
    const float ax = mx - s.v1x, ay = my - s.v1y;
    const float bx = s.v2x - s.v1x, by = s.v2y - s.v1y;
    return ax * by - ay * bx < 0.0f;
}

// Steps 2 and 3: the sector whose floor shows at (mx, my), or -1 (background).
DG_HD int32_t floor_sector_of_leaf(const FloorTables &t, int32_t leaf, float mx, float my) {
    if (leaf < 0) return -1;
    const FloorLeaf l = t.leaves[leaf];
    if (l.sector < 0 || (uint32_t)l.sector >= t.n_sectors || l.first > t.n_segs || l.count > t.n_segs - l.first) return -1;
    for (uint32_t k = 0; k < l.count; k++)
        if (floor_behind(t.segs[l.first + k], mx, my)) return -1;
    return l.sector;
}
DG_HD int32_t floor_sector_at(const FloorTables &t, float mx, float my) { return floor_sector_of_leaf(t, floor_leaf_at(t, mx, my), mx, my); }

// Step 4: a sector's cell for one view from its flat handle (fs_core.h) and its light level: Flats::get_animated at the timestamp, a
// missing flat or a sky floor -1; the factor is diminish_color's at distance 0.
DG_HD FloorCell floor_cell(int32_t handle, const FsAnim *anims, uint32_t n_anims, uint32_t n_flats, float timestamp, int16_t light) {
    FloorCell c{-1, light_factor((float)light / 255.0f, 0)};
    if (handle < 0 || (handle & (FS_FLAT_MISSING | FS_FLAT_SKY))) return c;
    const int32_t anim = fs_handle_anim(handle);
    if (anim >= 0 && ((uint32_t)anim >= n_anims || anims[anim].n < 1 || anims[anim].n > 4)) return c;
    const int32_t flat = fs_resolve_flat(fs_handle_flat(handle), anim, anims, timestamp);
    if (flat >= 0 && (uint32_t)flat < n_flats) c.flat = flat;
    return c;
}

// Step 5: the texel's place in a flat.
DG_HD uint32_t floor_texel(float mx, float my) {
    const int32_t tx = f32_as_i32(floorf(mx)) & 63, ty = f32_as_i32(floorf(my)) & 63;
    return (uint32_t)ty * 64u + (uint32_t)tx;
}

// Steps 4 and 5 on the device and the host alike: the owner-tile word of a pixel that no line covers — 0 (background) or FLOOR_VALUE |
// RGB24.  row: the frame's cells [n_sectors]; seen: the frame's sector bits, or null (every sector is shown).
DG_HD uint32_t floor_value(const FloorTables &t, int32_t sector, const FloorCell *row, const uint32_t *seen, float mx, float my) {
    if (sector < 0) return 0u;
    if (seen && !((seen[(uint32_t)sector >> 5] >> ((uint32_t)sector & 31u)) & 1u)) return 0u;
    const FloorCell c = row[sector];
    if (c.flat < 0 || (uint32_t)c.flat >= t.n_flats) return 0u;
    const uint32_t texel = t.flats[(size_t)c.flat * 4096u + floor_texel(mx, my)];
    return FLOOR_VALUE | shade(t.palette[texel], c.factor);
}

// The pixel (X, Y) of a frame whose owner tile holds no line there.
DG_HD uint32_t floor_pixel(const FloorTables &t, const FloorCell *row, const uint32_t *seen, int32_t X, int32_t Y, int32_t W, int32_t H, const EgoView &v,
                           float inv, bool rotate) {
    float mx, my;
    floor_map_point(X, Y, W, H, v, inv, rotate, mx, my);
    return floor_value(t, floor_sector_at(t, mx, my), row, seen, mx, my);
}

// An owner-tile word as RGB24: a floor pixel's own colour, else the line's (ego_value_rgb).
DG_HD uint32_t floor_value_rgb(uint32_t v) { return (v & FLOOR_VALUE) ? (v & 0xffffffu) : ego_value_rgb(v); }

// With a mask: linedef l's bit set in the frame's mask row shows the sectors of both its sidedefs.
DG_HD bool floor_seen_line(const uint32_t *mask_row, uint32_t l) { return ((mask_row[l >> 5] >> (l & 31u)) & 1u) != 0u; }

}  // namespace dg
