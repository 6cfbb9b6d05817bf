// map_things_core.h — the rules of the map-object markers on the player-centred and floor-textured map frames as
// host/device inline functions: which edges a marker has, where they lie in map space, the owner-tile value of an edge and its colour.
// map_things_kernels.hip runs them on the GPU (ego_tile_things.h), map_things_host.hpp on the host (dg_map_thing_lines,
// dg_ego_map_things_host, dg_floor_map_things_host), and tests/map_things/map_things_host_main.cpp runs the things phase as a host loop
// over the same functions against the literal rule.
//
// A shown object at (x, y) with R = (float)radius and (ca, sa) = (cosf(angle), sinf(angle)) from the host's libm has up to five edges, every
// operation in f32, no contraction:
//     0..3  the box (DG_MARK_BOX): c0 = (x-R, y-R), c1 = (x+R, y-R), c2 = (x+R, y+R), c3 = (x-R, y+R); c0->c1, c1->c2, c2->c3, c3->c0
//     4     the heading (DG_MARK_HEADING): (x, y) -> (x + R*ca, y + R*sa); an angle that is not finite (ca or sa not within +-1) has none
// Every endpoint goes through ego_point unchanged.  A shown object has |x|, |y| <= 32768 and R <= 1024, |ca|, |sa| <= 1, so an endpoint lies
// within +-33792 of the origin; with |view.x|, |view.y| <= 65536 that is |r|, |f| <= 2 * 99328 (ego_core.h has the same sum with 98304 for
// a WAD vertex), times a scale of at most 64 plus 8192: 12 722 176 + rounding < 2^24 = 16 777 216.  map_seg_make's precondition holds for
// every marker edge of every in-contract view, translated by a band's first row (< 16384) too.
//
// The owner-tile value of edge e of object i is THING_VALUE | i << 3 | e: above every linedef's (at most 131 071), below the arrow's
// (EGO_ARROW_VALUE), without the floor's bit (FLOOR_VALUE), and increasing in draw order — objects in index order, box edges, then heading.
#pragma once
#include <cmath>

#include "ego_core.h"

namespace dg {

constexpr uint32_t THING_MAX = 65536u;                    // map objects of a scene with markers: i << 3 | e stays below THING_VALUE
constexpr uint32_t THING_EDGES = 5u;                      // items per object: four box edges and the heading
constexpr uint32_t THING_VALUE = 0x20000000u;             // tile word of a marker edge: this bit | object << 3 | edge
constexpr uint32_t THING_KIND = 0xe0000000u;              // ... told from a linedef's, the arrow's and a floor pixel's by these three bits
constexpr uint32_t MARK_BOX = 1u, MARK_HEADING = 2u;      // DG_MARK_*
constexpr int32_t THING_MAX_RADIUS = 1024;
constexpr float THING_MAX_COORD = 32768.0f;

struct ThingMarker { float radius; uint32_t rgb, flags; };          // dg_map_marker as the kernels read it: R converted once
static_assert(sizeof(ThingMarker) == 12, "ThingMarker");
struct ThingPlace { float x, y, ca, sa; };                          // an object as loaded: position, cosf / sinf of its angle
static_assert(sizeof(ThingPlace) == 16, "ThingPlace");
struct ThingEntry { int32_t mobj; float x, y, ca, sa; };            // a frame's pose of one object, after later-wins
static_assert(sizeof(ThingEntry) == 20, "ThingEntry");

DG_HD uint32_t thing_value(uint32_t object, uint32_t edge) { return THING_VALUE | (object << 3) | edge; }
DG_HD bool thing_is_value(uint32_t v) { return (v & THING_KIND) == THING_VALUE; }
DG_HD uint32_t thing_value_object(uint32_t v) { return (v & ~THING_KIND) >> 3; }
// The colour of a tile word that is a marker edge's (an object beyond the table: black — never, the values come from the table's indices).
DG_HD uint32_t thing_value_rgb(uint32_t v, const ThingMarker *markers, uint32_t n_things) {
    const uint32_t i = thing_value_object(v);
    return i < n_things ? markers[i].rgb : 0u;
}

// A position a marker is drawn at: finite, within the map's coordinate range.  (A comparison with a NaN is false.)
DG_HD bool thing_position_ok(float x, float y) { return fabsf(x) <= THING_MAX_COORD && fabsf(y) <= THING_MAX_COORD; }

// Edge `edge` (0 .. THING_EDGES - 1) of the marker m of an object at p, in map space; false: the marker has no such edge.
DG_HD bool thing_edge(const ThingPlace &p, const ThingMarker &m, uint32_t edge, EgoLine &l) {
    const float R = m.radius;
    if (edge < 4u) {
        if (!(m.flags & MARK_BOX)) return false;
        const float xl = p.x - R, xh = p.x + R, yl = p.y - R, yh = p.y + R;
        if (edge == 0u) l = EgoLine{xl, yl, xh, yl};
        else if (edge == 1u) l = EgoLine{xh, yl, xh, yh};
        else if (edge == 2u) l = EgoLine{xh, yh, xl, yh};
        else l = EgoLine{xl, yh, xl, yl};
        return true;
    }
    if (!(m.flags & MARK_HEADING) || !(fabsf(p.ca) <= 1.0f && fabsf(p.sa) <= 1.0f)) return false;
    l = EgoLine{p.x, p.y, p.x + R * p.ca, p.y + R * p.sa};
    return true;
}

// Where object `mobj` is in a frame: its entry among the frame's n entries (sorted by object, one per object), else as loaded.
DG_HD ThingPlace thing_place(const ThingEntry *entries, uint32_t n, const ThingPlace *places, uint32_t mobj) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint32_t)entries[mid].mobj < mobj) lo = mid + 1u;
        else hi = mid;
    }
    if (lo < n && (uint32_t)entries[lo].mobj == mobj) return ThingPlace{entries[lo].x, entries[lo].y, entries[lo].ca, entries[lo].sa};
    return places[mobj];
}

DG_HD uint32_t thing_shown_words(uint32_t n_things) { return (n_things + 31u) / 32u; }
DG_HD bool thing_shown(const uint32_t *row, uint32_t mobj) { return ((row[mobj >> 5] >> (mobj & 31u)) & 1u) != 0u; }

// The things phase for one item: edge `edge` of object `mobj` of a frame, as a segment in the band's own coordinates (count 0: nothing
// to draw — not shown, no such edge, or it misses the band).
DG_HD MapSeg thing_band_seg(uint32_t mobj, uint32_t edge, const uint32_t *shown_row, const ThingMarker *markers, const ThingEntry *entries, uint32_t n_entries,
                            const ThingPlace *places, const EgoView &v, float scale, bool rotate, int32_t W, int32_t H, int32_t row0, int32_t rows) {
    MapSeg none{};
    if (!thing_shown(shown_row, mobj)) return none;
    const ThingMarker m = markers[mobj];
    EgoLine l;
    if (!thing_edge(thing_place(entries, n_entries, places, mobj), m, edge, l)) return none;
    return ego_band_seg(l, thing_value(mobj, edge), v, scale, rotate, W, H, row0, rows);
}

}  // namespace dg
