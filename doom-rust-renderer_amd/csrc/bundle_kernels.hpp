// bundle_kernels.hpp — launch interface between the context (host) and bundle_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "bundle_core.h"
#include "kernels.hpp"

namespace dg {

// What dg_bundle_tiles writes: the planes of the parts `what` names (BUNDLE_DEPTH: dist + kind, BUNDLE_LABELS: id + cls + boxes), each
// [n_frames][H][W]; the pointers of a part not asked for are not read.
struct BundlePlanes {
    int16_t *dist;
    uint8_t *kind;
    uint16_t *id;
    uint8_t *cls;
    LabelRawBox *boxes;          // [n_frames][n_mobjs], cleared by the launch (label_core.h; the host finishes an entry with label_box_finish)
    uint32_t n_mobjs;
};

// dg_bundle_tiles over every (frame, 64-column strip, band of rows) of the host lists P points at (frames, col_off, spans, walls, planes,
// the scene's opacity plane; P.rspans, P.fb and P.row_tab are not read), owners[] parallel to P.walls (read only with BUNDLE_LABELS; every
// map-object id in it must be below n_mobjs).  Every pixel of every requested plane is written.  `what` must name BUNDLE_DEPTH or
// BUNDLE_LABELS (BUNDLE_COLOUR is not this kernel's and is ignored).  start / stop: optional timing events attached to the dispatch
// (kernels.hpp); the clearing of the box rows is queued in front of start.
hipError_t launch_bundle(const RasterParams &P, const uint32_t *owners, const BundlePlanes &out, uint32_t what, hipStream_t stream,
                         hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
