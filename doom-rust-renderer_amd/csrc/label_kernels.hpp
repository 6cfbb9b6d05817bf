// label_kernels.hpp — launch interface between the context (host) and label_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "kernels.hpp"
#include "label_core.h"

namespace dg {

// The label frame of the host lists P points at (frames, col_off, spans, walls, the scene's opacity plane; P.planes, P.rspans, P.fb and
// P.row_tab are not read), owners[] parallel to P.walls:
//   dg_label_tiles  over every (frame, 64-column strip, band of rows): id[n_frames][H][W] and cls[n_frames][H][W], every pixel written;
//   dg_label_boxes  over the same decomposition: the planes reduced into boxes[n_frames][n_mobjs], which is cleared first (label_core.h:
//                   LabelRawBox; the host finishes an entry with label_box_finish).
// Every map-object id in owners[] must be below n_mobjs.  start / mid / stop: optional timing events attached to the dispatches
// (kernels.hpp): start .. mid spans dg_label_tiles, mid .. stop dg_label_boxes.
hipError_t launch_labels(const RasterParams &P, const uint32_t *owners, uint16_t *id, uint8_t *cls, LabelRawBox *boxes, uint32_t n_mobjs,
                         hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t mid = nullptr, hipEvent_t stop = nullptr);

}  // namespace dg
