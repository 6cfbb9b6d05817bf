// plane_reduce_core.h — reduced-size depth and label planes (dg_reduce_planes_*, dg_readback_planes_reduced*): which
// source pixel represents a box, as one body for the host path (dg_reduce_planes_host, api_scene.cpp) and the device path
// (plane_reduce_kernels.hip).  The box geometry is reduce_core.h's.  Integer arithmetic only.
#pragma once
#include "reduce_core.h"

namespace dg {

// What a descriptor has to be.
DG_HD bool plane_reduce_desc_ok(const dg_plane_reduce_desc &d) {
    return d.fx >= 1u && d.fx <= REDUCE_MAX_FACTOR && d.fy >= 1u && d.fy <= REDUCE_MAX_FACTOR &&
           (d.rule == DG_PLANE_POINT || d.rule == DG_PLANE_NEAREST) && d.reserved == 0u;
}

// DG_PLANE_POINT: the pixel in the middle of a whole box, clamped into the frame for a short box at an edge.
DG_HD uint32_t plane_point(uint32_t o, uint32_t f, uint32_t extent) {
    const uint32_t p = o * f + f / 2u;
    return p < extent ? p : extent - 1u;
}

// DG_PLANE_NEAREST.  The order of the rule — smallest signed distance, then lowest row, then lowest column — is the unsigned order of
//   key = ((d ^ 0x8000) & 0xFFFF) << 8 | ry << 4 | rx        (ry, rx: row and column inside the box, each < 16)
// because flipping the sign bit maps the int16 order onto the uint16 order.  The minimum is taken in two steps that both keep that
// order: over the rows of one column with the row in the low bits (plane_col_key), then over the columns of the box with the column
// appended below (plane_box_key).
DG_HD uint32_t plane_col_key(uint32_t d16, uint32_t ry) { return (((d16 ^ 0x8000u) & 0xFFFFu) << 4) | ry; }
DG_HD uint32_t plane_box_key(uint32_t col_key, uint32_t rx) { return (col_key << 4) | rx; }
constexpr uint32_t PLANE_KEY_NONE = 0xFFFFFFFFu;    // above every key: the start of a minimum
DG_HD uint32_t plane_key_rx(uint32_t key) { return key & 15u; }
DG_HD uint32_t plane_key_ry(uint32_t key) { return (key >> 4) & 15u; }
DG_HD int16_t plane_key_distance(uint32_t key) { return (int16_t)(uint16_t)((key >> 8) ^ 0x8000u); }

// The key of box [x0, x0 + nx) x [y0, y0 + ny) of a distance plane of width W: the serial form of the rule.
DG_HD uint32_t plane_nearest_key(const int16_t *distance, uint32_t W, uint32_t x0, uint32_t nx, uint32_t y0, uint32_t ny) {
    uint32_t best = PLANE_KEY_NONE;
    for (uint32_t rx = 0; rx < nx; rx++) {
        uint32_t col = PLANE_KEY_NONE;
        for (uint32_t ry = 0; ry < ny; ry++) {
            const uint32_t k = plane_col_key((uint16_t)distance[(size_t)(y0 + ry) * W + x0 + rx], ry);
            col = k < col ? k : col;
        }
        const uint32_t k = plane_box_key(col, rx);
        best = k < best ? k : best;
    }
    return best;
}

}  // namespace dg
