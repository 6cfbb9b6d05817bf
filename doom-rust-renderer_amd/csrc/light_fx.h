// light_fx.h — the sector light effects (dg_scene_set_light_effects): the level the reference's sector thinkers
// (src/lights.rs, set up by init_sector_thinkers in src/thinkers.rs) leave in a sector after `tics` calls of mutate(), as one body for the
// host walker (frontend.cpp), dg_scene_sector_lights_at (context.cpp) and the device rows of the seg walk (light_fx_kernels.hip).
// Integer arithmetic only: i16 levels wrap as in the reference's release build.  No loop's bound depends on the timestamp: glow and strobe
// are closed forms, flash and fire cost one table search and at most 64 draws.
#pragma once
#include "../../include/doomgpu.h"
#include "fs_core.h"

namespace dg {

enum : uint8_t { LFX_FLASH = 1, LFX_GLOW = 8, LFX_FIRE = 17 };   // every other record is a strobe (2, 3, 4, 12, 13)

// One effect sector.  min / max as init_thinkers computes them on the freshly loaded map (the WAD's levels); dark: the strobe's dark
// time D; c0: the strobe's first switch tic; tab: word offset of the flash / fire tables in the scene's table array.
struct LfxRec { uint32_t sector; uint8_t type, dark; uint16_t c0; int16_t min, max; uint32_t tab; };
static_assert(sizeof(LfxRec) == 16, "LfxRec layout");

constexpr uint32_t LFX_PERIOD_DRAWS = 4096;     // the draw index runs mod this: flash and fire repeat after 4096 durations / steps
constexpr uint32_t LFX_CHECKPOINT = 64;         // table checkpoints every 64 durations / steps
constexpr uint32_t LFX_FLASH_WORDS = 65;        // S_{64j}, j = 0 .. 64 (the last one: the period in tics)
constexpr uint32_t LFX_FIRE_BYTES = 20 + 5 + 5 * 64;   // transition [level][draw], period map [level], checkpoints [start level][64]
constexpr uint32_t LFX_FIRE_WORDS = (LFX_FIRE_BYTES + 3) / 4;

DG_HD uint64_t lfx_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The stand-in for the reference's ThreadRng draws: a value in [0, n) of stream 1 (flash), 2 (strobe phase) or 3 (fire).
DG_HD uint32_t lfx_draw(uint64_t seed, uint32_t stream, uint32_t sector, uint32_t index, uint32_t n) {
    const uint64_t key = 1ull + (((uint64_t)stream << 48) | ((uint64_t)sector << 32) | (uint64_t)index);
    return (uint32_t)(((lfx_mix64(seed + 0x9E3779B97F4A7C15ull * key) >> 32) * (uint64_t)n) >> 32);
}
DG_HD int16_t lfx_wrap(uint32_t v) { return (int16_t)(uint16_t)v; }

// GlowingLight::mutate (lights.rs:190-211) from max, going down first, in closed form.  m: the down steps before the first turn,
// b: the level of the turn.  The usual orbit is max, max-8, .., b, then a triangle of period 2m between b and max-8.  When the down
// test at b wraps below -32768 the level walks down through its residue class for ever; when max+8 wraps above 32767 (m = 0) it walks
// up once through the class and settles at max-8.
DG_HD int16_t lfx_glow(int32_t mn, int32_t mx, uint32_t T) {
    const int32_t m = mx - mn > 8 ? (mx - mn - 1) >> 3 : 0, b = mx - 8 * m;
    if (b - 8 < -32768) {
        if (mn < mx || T < 8191u) return lfx_wrap((uint32_t)mx - 8u * T);
        return (int16_t)(mx + 8);                               // min == max < -32760: stuck one step above after 8191 tics
    }
    if (m == 0) {
        if (mx + 8 <= 32767 || T <= 1u) return (int16_t)mx;
        return T <= 8192u ? lfx_wrap((uint32_t)mx + 8u * (T - 1u)) : (int16_t)(mx - 8);
    }
    if (T <= (uint32_t)m) return (int16_t)(mx - 8 * (int32_t)T);
    const uint32_t u = (T - (uint32_t)m - 1u) % (2u * (uint32_t)m);
    const int32_t tri = u < (uint32_t)m ? (int32_t)u : (u == (uint32_t)m ? m - 1 : 2 * m - 1 - (int32_t)u);
    return (int16_t)(b + 8 * tri);
}

// StrobeFlash (lights.rs:99-156): max before the first switch at c0, then D tics at min and B = 5 at max, in turn.
DG_HD int16_t lfx_strobe(const LfxRec &r, uint32_t T) {
    if (T < r.c0) return r.max;
    return (T - r.c0) % ((uint32_t)r.dark + 5u) < r.dark ? r.min : r.max;
}

// LightFlash (lights.rs:44-97): durations d_k = 1 + draw(1, s, k mod 4096, k even ? 64 : 7) alternate bright and dark; the level is max
// when an even number of switches S_k = d_0 + .. + d_{k-1} (k >= 1) lie at or before T.  tab: S_{64j}, j = 0 .. 64.
DG_HD int16_t lfx_flash(const LfxRec &r, const uint32_t *tab, uint64_t seed, uint32_t T) {
    T %= tab[64];
    uint32_t j = 0;
    for (uint32_t step = 32; step; step >>= 1)
        if (tab[j + step] <= T) j += step;
    uint32_t S = tab[j], k = j * LFX_CHECKPOINT;
    for (uint32_t i = 0; i < LFX_CHECKPOINT; i++) {
        const uint32_t d = 1u + lfx_draw(seed, 1u, r.sector, k, (k & 1u) ? 7u : 64u);
        if (S + d > T) break;
        S += d; k++;
    }
    return (k & 1u) ? r.min : r.max;
}

// FireFlicker (lights.rs:213-259): step j at tic 4j draws a = 16 * draw(3, s, j mod 4096, 4).  The level is one of five: index i < 4
// is max - 16 i, index 4 is min.  tab (bytes): trans[5][4], the map of one period (4096 steps) [5], the level every 64 steps of a
// period from each start level [5][64].
DG_HD int16_t lfx_fire_level(const LfxRec &r, uint32_t x) { return x < 4u ? lfx_wrap((uint32_t)(int32_t)r.max - 16u * x) : r.min; }
DG_HD int16_t lfx_fire(const LfxRec &r, const uint8_t *tab, uint64_t seed, uint32_t T) {
    const uint8_t *trans = tab, *pmap = tab + 20, *cp = tab + 25;
    const uint32_t J = T >> 2, P = J / LFX_PERIOD_DRAWS, rem = J % LFX_PERIOD_DRAWS;
    uint32_t x = 0;                                             // P periods: the orbit of max under the period map (5 states)
    for (uint32_t i = 0; i < 5u; i++)
        if (i < P) x = pmap[x];
    if (P > 5u) {                                               // x is on the cycle: reduce the rest of P by its length
        uint32_t y = pmap[x], len = 1;
        for (uint32_t i = 0; i < 4u && y != x; i++) { y = pmap[y]; len++; }
        const uint32_t more = (P - 5u) % len;
        for (uint32_t i = 0; i < 4u; i++)
            if (i < more) x = pmap[x];
    }
    const uint32_t q = rem / LFX_CHECKPOINT;
    x = cp[x * 64u + q];
    for (uint32_t i = 0; i < rem % LFX_CHECKPOINT; i++)
        x = trans[x * 4u + lfx_draw(seed, 3u, r.sector, (q * LFX_CHECKPOINT + 1u + i) % LFX_PERIOD_DRAWS, 4u)];
    return lfx_fire_level(r, x);
}

// The effect's level after `tics` mutate() calls.
DG_HD int16_t lfx_level(const LfxRec &r, const uint32_t *tab, uint64_t seed, uint32_t tics) {
    if (r.type == LFX_GLOW) return lfx_glow(r.min, r.max, tics);
    if (r.type == LFX_FLASH) return lfx_flash(r, tab + r.tab, seed, tics);
    if (r.type == LFX_FIRE) return lfx_fire(r, reinterpret_cast<const uint8_t *>(tab + r.tab), seed, tics);
    return lfx_strobe(r, tics);
}

// dg_light_rows' arguments: the seg walk's light rows [n_frames][n_sectors] from a base row (base_stride 0) or per-view rows
// (base_stride n_sectors; out may be base), each effect sector replaced by its level at the view's tics unless the view's override
// mask (mask_words words per frame, nullptr: none) has its bit.
struct LfxRows {
    const LfxRec *recs; const uint32_t *tab; const int32_t *rec_of;     // rec_of: per sector its record or -1
    const dg_view *views;
    const int16_t *base; const uint32_t *mask;
    int16_t *out;
    uint64_t seed;
    uint32_t n_sectors, base_stride, mask_words;
    int n_frames;
};

}  // namespace dg
