// overlay_core.h — screen pictures over finished colour frames (dg_overlay_host / _device, dg_slot_overlay): the rule
// of one item, as host/device inline functions, and the records the host resolves a call's items into.  The host twin (api_scene.cpp) and
// the kernel (overlay_kernels.hip) evaluate the same functions on the same records; overlay_plan.hpp makes the records.
//
//   Pictures::get          src/graphics/pictures.rs:38-47     the picture of a name (Scene::use_picture)
//   Bitmap::test_flat_draw src/graphics/bitmap.rs:28-53       one palette-coloured scale x scale rectangle per Some texel
//   Picture::mirror        src/graphics/pictures.rs:129-147   texel column w-1-tx
//   diminish_color         src/renderer/bitmap_render.rs:190-208, at distance 0 (raster_core.h's light_factor / shade)
//
// Everything but the shade is integer arithmetic.  A pixel's texel column is (px - ox) / scale_x with px - ox < 32767 * 16 < 2^19 and
// the scale in 1..16: ovl_div does it with one multiply (ovl_magic), exact on that domain — tests/overlay/overlay_host_main.cpp
// enumerates it.
#pragma once
#include "../../include/doomgpu.h"
#include "raster_core.h"

namespace dg {

constexpr int32_t OVL_MAX_SCALE = 16, OVL_MAX_XY = 1 << 20;
constexpr uint32_t OVL_TILE_W = 64, OVL_TILE_H = 16;      // a workgroup's tile: one wave per row, four rows per wave
constexpr uint32_t OVL_LANES = 256;
constexpr uint32_t OVL_TILES_PER_RECT = 64;               // a rectangle record names at most this many tiles (overlay_plan.hpp splits)

// A picture as an item names it: a bitmap of the scene (column-major planes at texel_off) with its offsets.
struct OvlPicture { int32_t w, h, left, top; uint32_t texel_off; };

// One item, resolved against its picture and clipped to the frame: x0 <= px < x1, y0 <= py < y1 is what it covers (never empty).
struct OvlItem {
    int32_t x0, y0, x1, y1;
    int32_t ox, oy;                  // the unclipped origin: ox <= x0, oy <= y0
    uint32_t texel_off, h;           // texel (tx, ty) of the picture: texel_off + tx * h + ty
    int32_t tx_at, tx_step;          // the picture's column of scaled column c: tx_at + tx_step * c  (0, 1; mirrored: w - 1, -1)
    uint32_t mx, my;                 // ovl_magic of the two scales
    float factor;                    // light_factor(light_level / 255, 0)
    uint32_t pad[3];
};
static_assert(sizeof(OvlItem) == 64, "OvlItem is read as sixteen words, on a 64-byte boundary of the staging");

// A rectangle of one frame that the items [item0, item1) of that frame may touch, cut into OVL_TILE_W x OVL_TILE_H tiles, row-major:
// this record stands for the tiles [tile0, tile0 + tiles) of them.  The rectangles of a frame are disjoint.
struct OvlRect {
    uint32_t frame;
    uint32_t x0, y0, x1, y1;         // 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H
    uint32_t item0, item1;
    uint32_t tile0, tiles, tiles_x;
};
static_assert(sizeof(OvlRect) == 40, "OvlRect is read as ten words (whole words: a scalar load reads no less)");

DG_HD bool ovl_item_ok(const dg_screen_picture &it, int32_t n_pictures) {
    return it.picture >= 0 && it.picture < n_pictures && it.scale_x >= 1 && it.scale_x <= OVL_MAX_SCALE && it.scale_y >= 1 && it.scale_y <= OVL_MAX_SCALE &&
           it.light_level >= 0 && it.light_level <= 255 && it.x >= -OVL_MAX_XY && it.x <= OVL_MAX_XY && it.y >= -OVL_MAX_XY && it.y <= OVL_MAX_XY &&
           (it.flags & ~(uint32_t)(DG_PIC_OFFSETS | DG_PIC_MIRROR)) == 0u;
}

// n / d for 0 <= n < 2^19, 1 <= d <= 16:  m = ceil(2^31 / d) = (2^31 + e) / d with 0 <= e < d, so 2 n m / 2^32 = n / d + n e / (d 2^31), and
// n e < 2^23 keeps the second term below 1 / d.
DG_HD uint32_t ovl_magic(uint32_t d) { return (0x80000000u + d - 1u) / d; }
DG_HD uint32_t ovl_div(uint32_t n, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n << 1, magic);
#else
    return (uint32_t)(((uint64_t)(n << 1) * magic) >> 32);
#endif
}

// The item of `it` on picture p in a W x H frame; false when it covers no pixel of the frame (`o` is then not an item).
DG_HD bool ovl_resolve(const dg_screen_picture &it, const OvlPicture &p, int32_t W, int32_t H, OvlItem &o) {
    const int32_t sx = it.scale_x, sy = it.scale_y;
    const bool offsets = (it.flags & DG_PIC_OFFSETS) != 0, mirror = (it.flags & DG_PIC_MIRROR) != 0;
    o.ox = it.x - (offsets ? p.left * sx : 0);           // |x| <= 2^20, |left * sx| < 2^19
    o.oy = it.y - (offsets ? p.top * sy : 0);
    const int32_t ex = o.ox + p.w * sx, ey = o.oy + p.h * sy;
    o.x0 = o.ox > 0 ? o.ox : 0; o.y0 = o.oy > 0 ? o.oy : 0;
    o.x1 = ex < W ? ex : W; o.y1 = ey < H ? ey : H;
    o.texel_off = p.texel_off; o.h = (uint32_t)p.h;
    o.tx_at = mirror ? p.w - 1 : 0; o.tx_step = mirror ? -1 : 1;
    o.mx = ovl_magic((uint32_t)sx); o.my = ovl_magic((uint32_t)sy);
    o.factor = light_factor((float)it.light_level / 255.0f, 0);
    o.pad[0] = o.pad[1] = o.pad[2] = 0u;
    return o.x0 < o.x1 && o.y0 < o.y1;
}

DG_HD bool ovl_covers(const OvlItem &it, int32_t px, int32_t py) { return px >= it.x0 && px < it.x1 && py >= it.y0 && py < it.y1; }
// The texel of a pixel the item covers, as an offset into the planes: inside the picture's w * h texels, because 0 <= px - ox < w * scale_x.
DG_HD uint32_t ovl_texel(const OvlItem &it, int32_t px, int32_t py) {
    const int32_t tx = it.tx_at + it.tx_step * (int32_t)ovl_div((uint32_t)(px - it.ox), it.mx);
    return it.texel_off + (uint32_t)tx * it.h + ovl_div((uint32_t)(py - it.oy), it.my);
}
// The colour of a Some texel v under the item's light: r | g << 8 | b << 16.
DG_HD uint32_t ovl_colour(const OvlItem &it, uint32_t palette_rgbx) { return shade(palette_rgbx, it.factor); }

}  // namespace dg
