// plane_kernels.hpp — launch interface between the context (host) and plane_kernels.hip: the depth planes, the label planes and a
// bundle's planes of the host lists P points at (frames, col_off, spans, walls, planes, the scene's opacity plane; P.rspans, P.fb and
// P.row_tab are not read).  Every plane is [n_frames][H][W], and every pixel of every plane a launch names is written.  The timing
// events are optional and attached to the dispatches themselves (kernels.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include "kernels.hpp"
#include "plane_core.h"

namespace dg {

// What dg_bundle_tiles writes: the planes of the parts `what` names (BUNDLE_DEPTH: dist + kind, BUNDLE_LABELS: id + cls + boxes); the
// pointers of a part not asked for are not read.
struct BundlePlanes {
    int16_t *dist;
    uint8_t *kind;
    uint16_t *id;
    uint8_t *cls;
    LabelRawBox *boxes;          // [n_frames][n_mobjs], cleared by the launch (label_core.h; the host finishes an entry with label_box_finish)
    uint32_t n_mobjs;
};

// dg_depth_tiles: dist and kind.  P.planes is read (a flat's wx).
hipError_t launch_depth(const RasterParams &P, int16_t *dist, uint8_t *kind, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// dg_label_tiles: id and cls, owners[] parallel to P.walls (P.planes is not read); then dg_label_boxes over the same decomposition: the
// planes reduced into boxes[n_frames][n_mobjs], which is cleared first.  Every map-object id in owners[] must be below n_mobjs.
// start .. mid spans dg_label_tiles, mid .. stop dg_label_boxes.
hipError_t launch_labels(const RasterParams &P, const uint32_t *owners, uint16_t *id, uint8_t *cls, LabelRawBox *boxes, uint32_t n_mobjs,
                         hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t mid = nullptr, hipEvent_t stop = nullptr);

// dg_bundle_tiles: the planes and the boxes of `out` in one walk.  owners[] is read only with BUNDLE_LABELS (every map-object id in it
// must be below n_mobjs).  `what` must name BUNDLE_DEPTH or BUNDLE_LABELS (BUNDLE_COLOUR is not this kernel's and is ignored).  The
// clearing of the box rows is queued in front of start.
hipError_t launch_bundle(const RasterParams &P, const uint32_t *owners, const BundlePlanes &out, uint32_t what, hipStream_t stream,
                         hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
