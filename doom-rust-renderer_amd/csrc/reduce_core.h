// reduce_core.h — reduced-size frames (dg_reduce_*, dg_readback_reduced*): the box bounds, the rounded divide and the
// luma of the box downscale, as one body for the host path (dg_reduce_host, api_scene.cpp) and the device path (reduce_kernels.hip).
// Integer arithmetic only: nothing here depends on the contraction setting.
#pragma once
#include "../../include/doomgpu.h"
#include "rust_num.h"

namespace dg {

constexpr uint32_t REDUCE_MAX_FACTOR = 16;          // dg_reduce_desc.fx / fy

// Output extent of a source extent under box size f: ceil(extent / f).
DG_HD uint32_t reduce_out_dim(uint32_t extent, uint32_t f) { return (extent + f - 1u) / f; }

// Box i of size f along an axis of `extent` source pixels: its first pixel; returns how many pixels of it exist (the last box of an
// axis that f does not divide is short).
DG_HD uint32_t reduce_box(uint32_t i, uint32_t f, uint32_t extent, uint32_t &lo) {
    lo = i * f;
    const uint32_t left = extent - lo;
    return left < f ? left : f;
}

// ceil(2^32 / 2n) for a box of n pixels, 1 <= n <= 256: what reduce_round multiplies by.  At most four n occur per call (interior,
// right edge, bottom edge, corner), so this — the one hardware division — runs on the host, four times per call.
DG_HD uint32_t reduce_rcp(uint32_t n) {
    const uint64_t d = 2ull * n;
    return (uint32_t)(((1ull << 32) + d - 1ull) / d);
}

// floor((2 s + n) / 2n): the mean of n bytes whose sum is s, rounded to nearest, halves up.  x = 2 s + n < 2^17 and the divisor is
// 2n <= 512, so with m = ceil(2^32 / 2n) = (2^32 + e) / 2n, e < 2n, the high word of x m is floor(x / 2n + x e / (2n 2^32)) and
// x e < 2^26 is too little to reach the next integer: exact (tests/test_reduce_host.py tries every x of every n).
DG_HD uint32_t reduce_round(uint32_t s, uint32_t n, uint32_t rcp) {
    return (uint32_t)(((uint64_t)(2u * s + n) * rcp) >> 32);
}

// DG_REDUCE_GRAY8 of the three rounded bytes.
DG_HD uint32_t reduce_luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// What a descriptor has to be.
DG_HD bool reduce_desc_ok(const dg_reduce_desc &d) {
    return d.fx >= 1u && d.fx <= REDUCE_MAX_FACTOR && d.fy >= 1u && d.fy <= REDUCE_MAX_FACTOR &&
           (d.format == DG_REDUCE_RGB24 || d.format == DG_REDUCE_GRAY8) && d.reserved == 0u;
}

// Bytes of one reduced frame.
DG_HD size_t reduce_frame_bytes(uint32_t w, uint32_t h, const dg_reduce_desc &d) {
    return (size_t)reduce_out_dim(w, d.fx) * (size_t)reduce_out_dim(h, d.fy) * (d.format == DG_REDUCE_GRAY8 ? 1u : 3u);
}

}  // namespace dg
