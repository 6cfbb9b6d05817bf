// depth_core.h — what a depth / surface-kind plane holds (include/doomgpu.h: dg_depth_*) and the one piece of arithmetic that is the
// depth frame's own, as a host/device inline function.  Which span writes a pixel, and the flats' wx: plane_core.h.
//
// The depth of a pixel is the `distance: i16` the reference hands to diminish_color for it (bitmap_render.rs:190-208):
//   wall / masked wall / sprite column : z                      src/renderer/bitmap_render.rs:251,267
//   floor / ceiling                    : wx as i16              src/renderer/visplanes.rs:113,126
//   sky, nothing                       : none — 32767 ("far")   src/renderer/visplanes.rs:74 writes the palette entry as it is
// Everything per column (texture column, the holes flag, the flat numerator) and every texel row comes from raster_core.h; the only
// arithmetic stated here is z (resolve_wall_span folds it into the light factor and drops it).
#pragma once
#include "raster_core.h"

namespace dg {

// include/doomgpu.h DG_KIND_*: the draw call that wrote the pixel last
enum : uint32_t { KIND_NONE = 0, KIND_COLUMN = 1, KIND_FLAT = 2, KIND_SKY = 3 };
constexpr int32_t DEPTH_FAR = 32767;          // the distance of a pixel nothing with a distance wrote

// z of bitmap_render.rs:251 — resolve_wall_span's expression, operand for operand.
DG_HD int32_t wall_distance(const DevSpan &sp, const DevWallRec &r) {
    float ax = (float)((int32_t)sp.x - r.start_x) / r.dxf;
    float oma = 1.0f - ax;
    float den = oma * r.C + ax * r.D;
    return f32_as_i16((oma + ax) / den);
}

}  // namespace dg
