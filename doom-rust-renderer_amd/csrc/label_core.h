// label_core.h — what an object-label plane and a box table hold (include/doomgpu.h: dg_label_*), as host/device inline functions.
//
// A pixel's label is the owner of the draw call that wrote it last; who writes is plane_core.h's question.  What is written: the owner
// tag of the span's draw record (owners[], parallel to the frame's walls[]) for a wall, masked wall or sprite column, the bare class for
// a floor / ceiling or the sky.
#pragma once
#include "raster_core.h"

namespace dg {

// include/doomgpu.h DG_LABEL_*
enum : uint32_t { LABEL_NONE = 0, LABEL_WALL = 1, LABEL_MOBJ = 2, LABEL_FLAT = 3, LABEL_SKY = 4 };

DG_HD uint32_t label_class(uint32_t tag) { return tag >> 16; }
DG_HD uint32_t label_index(uint32_t tag) { return tag & 0xffffu; }
// A tag a caller may hand over: class wall or map object, the index inside the scene's table (this keeps the box table in bounds).
DG_HD bool label_tag_ok(uint32_t tag, uint32_t n_segs, uint32_t n_mobjs) {
    return (label_class(tag) == LABEL_WALL && label_index(tag) < n_segs) || (label_class(tag) == LABEL_MOBJ && label_index(tag) < n_mobjs);
}

// ---- boxes -----------------------------------------------------------------------------------------------------------------------------
// The box table while it is being reduced: five words per (frame, map object), all zero when nothing owns a pixel, every update an
// atomicAdd (the count) or an atomicMax of a value that is at least 1 — so one memset clears it and the order of the updates cannot
// matter.  The minima are kept as maxima of their distance from the far edge.
constexpr uint32_t LABEL_BOX_WORDS = 5;       // pixels | x1 + 1 | y1 + 1 | W - x0 | H - y0
struct LabelRawBox { uint32_t w[LABEL_BOX_WORDS]; };

// include/doomgpu.h dg_label_box from a reduced entry (x0, y0, x1, y1 = -1 when no pixel).
DG_HD void label_box_finish(const LabelRawBox &r, int32_t W, int32_t H, uint32_t &pixels, int32_t &x0, int32_t &y0, int32_t &x1, int32_t &y1) {
    pixels = r.w[0];
    if (pixels == 0) { x0 = y0 = x1 = y1 = -1; return; }
    x1 = (int32_t)r.w[1] - 1; y1 = (int32_t)r.w[2] - 1;
    x0 = W - (int32_t)r.w[3]; y0 = H - (int32_t)r.w[4];
}

}  // namespace dg
