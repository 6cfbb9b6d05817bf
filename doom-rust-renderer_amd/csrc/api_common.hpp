// api_common.hpp — what the files that implement the C-ABI share: the calling thread's error string and the scene handle.
#pragma once
#include <string>

#include "../../include/doomgpu.h"
#include "binner.hpp"
#include "observe_core.h"
#include "overlay_plan.hpp"
#include "plane_reduce_core.h"
#include "scene.hpp"

extern thread_local std::string t_err;          // what dg_last_error reports (defined next to it, in api_scene.cpp)
inline int set_err(int code, const std::string &m) { t_err = m; return code; }

struct dg_scene { dg::Scene *sc; };

// What every reduced-planes call checks first (dg_plane_reduced_size, dg_reduce_planes_host / _device; the readbacks take the frame
// size from their ctx): the descriptor, the frame size, the frame count.
inline int check_plane_reduce(int width, int height, int n_frames, const dg_plane_reduce_desc *desc) {
    if (!desc) return set_err(DG_ERR_INVALID, "null argument");
    if (!dg::plane_reduce_desc_ok(*desc)) return set_err(DG_ERR_INVALID, "plane reduce descriptor: fx and fy in 1..16, a known rule, reserved 0");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384]");
    if (n_frames < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    return DG_OK;
}
// ... and of its eight planes: a source and its destination come together, and DG_PLANE_NEAREST needs the distance plane.
inline int check_plane_pairs(const dg_plane_reduce_desc &desc, const void *distance, const void *kind, const void *id, const void *cls,
                             const void *o_distance, const void *o_kind, const void *o_id, const void *o_cls) {
    if (!distance != !o_distance || !kind != !o_kind || !id != !o_id || !cls != !o_cls)
        return set_err(DG_ERR_INVALID, "a source plane without its destination, or a destination without its source");
    if (desc.rule == DG_PLANE_NEAREST && !distance) return set_err(DG_ERR_INVALID, "DG_PLANE_NEAREST needs the distance plane");
    return DG_OK;
}

// What dg_observed_size, dg_observe_host and dg_observe_device check alike, in this order: the descriptor, the frame size.
inline int check_observe(int width, int height, const dg_obs_desc *desc) {
    if (!desc) return set_err(DG_ERR_INVALID, "null argument");
    if (!dg::obs_desc_ok(*desc))
        return set_err(DG_ERR_INVALID, "observation descriptor: fx and fy in 1..16, a known source, rule (0 for colour) and dtype, reserved 0, "
                                       "lo <= hi inside int16, finite scale and bias, and for DG_OBS_U8 scale 1, bias 0, 0 <= lo, hi <= 255");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384]");
    return DG_OK;
}
// ... and the two that write, after it: the frame count, the pointers and their alignment, the strides.
inline int check_observe_call(const void *src, int width, int height, int n_frames, const dg_obs_desc *desc, const void *dst, const int64_t strides[4]) {
    const int rc = check_observe(width, height, desc);
    if (rc) return rc;
    if (!src || !dst || !strides) return set_err(DG_ERR_INVALID, "null argument");
    if (n_frames < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    if (desc->source == DG_OBS_DISTANCE && reinterpret_cast<uintptr_t>(src) % 2u) return set_err(DG_ERR_INVALID, "observe: a distance source must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(dst) % dg::obs_element_bytes(desc->dtype)) return set_err(DG_ERR_INVALID, "observe: dst must be aligned to its element size");
    const uint32_t extent[4] = {(uint32_t)n_frames, dg::obs_channels(desc->source), dg::reduce_out_dim((uint32_t)height, desc->fy), dg::reduce_out_dim((uint32_t)width, desc->fx)};
    if (!dg::obs_strides_ok(strides, extent))
        return set_err(DG_ERR_INVALID, "observe: every stride >= 1 and, sorted, each >= the one before times its extent (no two elements share an address)");
    return DG_OK;
}

// The scene's screen pictures as the overlay's items name them (dg_overlay_host: the scene's own; dg_upload_scene: the ctx's copy).
inline std::vector<dg::OvlPicture> overlay_pictures(const dg::Scene &sc) {
    std::vector<dg::OvlPicture> out;
    out.reserve(sc.pictures.size());
    for (const int32_t id : sc.pictures) {
        const dg::BitmapInfo &b = sc.bitmaps[(size_t)id];
        out.push_back(dg::OvlPicture{b.w, b.h, b.left_offset, b.top_offset, b.texel_off});
    }
    return out;
}
// What dg_overlay_host, dg_overlay_device and dg_slot_overlay check alike, and the plan of a call that passed.
inline int overlay_checked_plan(const std::vector<dg::OvlPicture> &pictures, int width, int height, int n_frames, const dg_screen_picture *items, const uint32_t *first,
                                dg::OvlPlan &plan) {
    if (const char *bad = dg::overlay_check((int32_t)pictures.size(), width, height, n_frames, items, first)) return set_err(DG_ERR_INVALID, bad);
    dg::overlay_plan(pictures.data(), width, height, n_frames, items, first, plan);
    return DG_OK;
}

// What dg_seen_lines_host and dg_seen_lines_device check alike: the scene (label frames' limit included), the plane size, the frame
// count, the three pointers.
inline int check_seen_lines(const dg::Scene *sc, int width, int height, int n, const void *id, const void *cls, const void *seen) {
    if (!sc) return set_err(DG_ERR_INVALID, "null scene");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return set_err(DG_ERR_INVALID, "width/height must be in [1, 16384]");
    if (n < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    if (!id || !cls || !seen) return set_err(DG_ERR_INVALID, "null argument");
    std::string err;
    const int rc = dg::check_label_scene(*sc, err);
    return rc ? set_err(rc, err) : DG_OK;
}
// ... and dg_seen_accumulate_host and dg_slot_seen_lines: count frames as whole runs of run_len.
inline int check_seen_runs(int words, int count, int run_len) {
    if (words < 1) return set_err(DG_ERR_INVALID, "a seen row has at least one word");
    if (count < 0) return set_err(DG_ERR_INVALID, "bad frame count");
    if (run_len < 1 || count % run_len) return set_err(DG_ERR_INVALID, "the frames must be whole runs of run_len >= 1");
    return DG_OK;
}
