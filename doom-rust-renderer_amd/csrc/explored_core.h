// explored_core.h — the rules of the explored-map frames as host/device inline functions: which pixel of a label
// plane marks a linedef as seen, the running OR along a session, and which line of a map pixel's cover an explored frame shows.
// explored_kernels.hip runs them on the GPU, api_scene.cpp on the host (dg_seen_lines_host, dg_seen_accumulate_host), and
// tests/explored/explored_host_main.cpp compiles explored_pick on the CPU against the literal draw loop.
//
// Seen rows.  A row is uint32 seen[words], words = ceil(L / 32) for L linedefs: bit l & 31 of word l >> 5 stands for linedef l, the
// bits at and above L stay 0.  Linedef l is seen by a frame when one pixel has class DG_LABEL_WALL and the index of a seg of l.
//
// Cover.  One uint32 per map pixel, built once per uploaded scene and frame size from the drawn linedefs in LINEDEFS order:
//     0                          no line covers the pixel
//     bit 31 clear               one line covers it: an entry
//     bit 31 set                 two or more do: the low 31 bits are an offset into chains[], where a count is followed by one entry per
//                                covering line, the LATEST line first (the order in which a frame would show them)
// An entry is  linedef + 1, with bit 30 set for yellow (two-sided) — red otherwise.
#pragma once
#include "rust_num.h"

namespace dg {

constexpr uint32_t SEEN_LABEL_WALL = 1u;                  // DG_LABEL_WALL
constexpr uint32_t SEEN_MAX_SEG_WORDS = 2048u;            // the seg bitset of one workgroup: 65 536 segs, the limit of label frames
constexpr uint32_t EXPLORED_MAX_WORDS = 2048u;            // a mask row as the frame kernel stages it: 65 536 linedefs
constexpr uint32_t EXPLORED_CHAIN = 0x80000000u, EXPLORED_YELLOW = 0x40000000u, EXPLORED_LINE = 0x3fffffffu;
constexpr uint32_t EXPLORED_RED_RGB = 0x0000ffu, EXPLORED_YELLOW_RGB = 0x00ffffu;   // r | g << 8 | b << 16, the map view's two colours

DG_HD uint32_t seen_words(uint32_t n_lines) { return (n_lines + 31u) / 32u; }
// Does a pixel of class `cls` and index `id` name a seg of a scene with n_segs segs?  (Any other class is ignored whatever its id.)
DG_HD bool seen_pixel(uint32_t cls, uint32_t id, uint32_t n_segs) { return cls == SEEN_LABEL_WALL && id < n_segs; }

DG_HD uint32_t popcount32(uint32_t v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}

DG_HD uint32_t explored_entry(uint32_t line, bool yellow) { return (line + 1u) | (yellow ? EXPLORED_YELLOW : 0u); }
DG_HD uint32_t explored_entry_rgb(uint32_t e) { return (e & EXPLORED_YELLOW) ? EXPLORED_YELLOW_RGB : EXPLORED_RED_RGB; }
DG_HD bool explored_entry_seen(uint32_t e, const uint32_t *mask_row) {
    const uint32_t line = (e & EXPLORED_LINE) - 1u;
    return (mask_row[line >> 5] >> (line & 31u)) & 1u;
}

// The colour (r | g << 8 | b << 16) an explored frame shows at a pixel whose cover word is `cover`: that of the latest line covering
// the pixel whose bit is set in mask_row, black when there is none.
DG_HD uint32_t explored_pick(uint32_t cover, const uint32_t *chains, const uint32_t *mask_row) {
    if (cover == 0u) return 0u;
    if (!(cover & EXPLORED_CHAIN)) return explored_entry_seen(cover, mask_row) ? explored_entry_rgb(cover) : 0u;
    const uint32_t *chain = chains + (cover & ~EXPLORED_CHAIN);
    const uint32_t n = chain[0];
    for (uint32_t i = 1; i <= n; i++) {
        const uint32_t e = chain[i];
        if (explored_entry_seen(e, mask_row)) return explored_entry_rgb(e);
    }
    return 0u;
}

}  // namespace dg
