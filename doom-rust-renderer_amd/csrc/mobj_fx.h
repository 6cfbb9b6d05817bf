// mobj_fx.h — the map-object state machine (dg_scene_set_mobj_thinkers): the state the reference's MapObjectThinker
// (src/map_objects.rs:62-121, set up by init_map_obj_thinkers in src/thinkers.rs) shows after `tics` calls of mutate(), with the
// everything-events (kill, explode, respawn) in between, as one body for the host walker (frontend.cpp), dg_scene_mobj_states_at
// (context.cpp) and the device rows of the seg walk (mobj_fx_kernels.hip).
// A chain is what mutate() walks from one start state, flattened by Scene::set_mobj_thinkers as prefix + cycle; a chain that ends in a
// tics == -1 state has that state as a cycle of one step of period 1.  Every step holds the value build_batch_fs writes into the
// per-view rows (sprite_frame * 2 + full_bright, -1 for S_NULL) and the number of mutates after which it ends, counted from the start
// of the prefix or of the cycle; a state lasts max(1, tics) mutates.  No loop's bound depends on the timestamp: one search over the
// steps of the prefix or of the cycle, and one pass over the scene's events (at most MFX_MAX_EVENTS).
#pragma once
#include "../../include/doomgpu.h"
#include "fs_core.h"

namespace dg {

constexpr uint32_t MFX_MAX_EVENTS = 16;         // events per scene (dg_scene_mobj_event)
constexpr int MFX_MAX_STATES = 65536;           // rows of a caller's state table: 65536 * 32767 mutates still fit the u32 sums below

struct MfxStep { uint32_t end; int32_t val; };
// steps [off, off + n_prefix) then [off + n_prefix, off + n_prefix + n_cycle); n_cycle >= 1, period >= 1
struct MfxChain { uint32_t off, n_prefix, n_cycle, prefix_total, period, pad; };
// Per thing type that is driven, by dg_scene_mobj_event's `what` (0: the spawn chain, 3 = respawn: the same): the chain the event
// sends the object to, or -1: the event does not move it.
struct MfxType { int32_t chain[4]; };
struct MfxEvent { uint32_t tics, what; };
static_assert(sizeof(MfxStep) == 8 && sizeof(MfxChain) == 24 && sizeof(MfxType) == 16 && sizeof(MfxEvent) == 8, "mobj_fx.h layouts");

// A map-object state as one value (host side; the device reads it in fs_ph_mobj): sprite_frame * 2 + full_bright, -1 for S_NULL.
inline int32_t mfx_encode(int32_t sprite_frame, int32_t full_bright) { return sprite_frame < 0 ? -1 : sprite_frame * 2 + (full_bright ? 1 : 0); }
inline void mfx_decode(int32_t v, int32_t &sprite_frame, int32_t &full_bright) {
    sprite_frame = v < 0 ? -1 : v >> 1;
    full_bright = v < 0 ? 0 : v & 1;
}

// The value of chain c after m mutates.
DG_HD int32_t mfx_chain_value(const MfxChain &c, const MfxStep *steps, uint32_t m) {
    const MfxStep *p = steps + c.off;
    uint32_t n = c.n_prefix;
    if (m >= c.prefix_total) { m = (m - c.prefix_total) % c.period; p += c.n_prefix; n = c.n_cycle; }
    uint32_t lo = 0;                                            // the first step with end > m (the last step's end is the total, > m)
    while (n > 1u) {
        const uint32_t half = n >> 1;
        if (p[lo + half - 1u].end <= m) { lo += half; n -= half; } else n = half;
    }
    return p[lo].val;
}

// The value of an object of type t after `tics` mutates: the last event at or before `tics` that moves it (none: spawned at 0) starts
// its chain, which then runs for the mutates since.  An event at E acts after the E-th mutate; events are in non-decreasing order.
DG_HD int32_t mfx_value(const MfxType &t, const MfxEvent *events, uint32_t n_events, const MfxChain *chains, const MfxStep *steps, uint32_t tics) {
    int32_t c = t.chain[0];
    uint32_t E = 0;
    for (uint32_t k = 0; k < n_events; k++) {
        const int32_t ck = t.chain[events[k].what & 3u];
        if (events[k].tics <= tics && ck >= 0) { c = ck; E = events[k].tics; }
    }
    return mfx_chain_value(chains[c], steps, tics - E);
}

// dg_mobj_rows' arguments: the seg walk's map-object rows [n_frames][n_mobjs] from a base row (base_stride 0) or per-view rows
// (base_stride n_mobjs; out may be base), each driven object replaced by its value at the view's tics unless the view's override
// mask (mask_words words per frame, nullptr: none) has its bit.
struct MfxRows {
    const MfxStep *steps; const MfxChain *chains; const MfxType *types; const MfxEvent *events;
    const int32_t *type_of;                                     // per map object its MfxType or -1 (not driven)
    const dg_view *views;
    const int32_t *base; const uint32_t *mask;
    int32_t *out;
    uint32_t n_events, n_mobjs, base_stride, mask_words;
    int n_frames;
};

}  // namespace dg
