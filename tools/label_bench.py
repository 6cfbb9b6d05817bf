#!/usr/bin/env python3
"""label_bench.py — label frames/s and the times of dg_label_tiles and dg_label_boxes next to dg_depth_tiles on one MI355X.

    python tools/label_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), as tools/depth_bench.py.
Label and depth submissions take the same host list route and walk the same spans, so dg_depth_tiles for the SAME views in the same run is
the yardstick of dg_label_tiles.  The two are measured in alternating rounds (label, depth, label, depth, ...) so that the spread between
rounds of one kernel can be held against the difference between the two.  Prints one JSON line:
  label_frames_per_s      frames / wall time of dg_submit_label_views + dg_wait, --batch frames per submission, two slots round robin
  label_host_ms           median host list generation of one submission (dg_timing.host_ms)
  label_tiles_ms,
  label_boxes_ms          median GPU time of each kernel over the --batch frames (dg_slot_label_timing: the events attached to the dispatches)
  depth_tiles_ms          median GPU time of dg_depth_tiles for the same views
  *_rounds                the per-round medians the figures above are the medians of: their range is the run-to-run spread
  boxes_read_gb_per_s     3 * W * H bytes per frame (the two planes) over label_boxes_ms
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)

    def loop(submit, iters, read):
        """-> (frames/s, [what read(slot) gives for every submission])"""
        seen = []
        t0 = time.perf_counter()
        for i in range(iters):
            if i >= 2:
                seen.append(read(i % 2))                       # (waits for the slot, as the next submission into it would)
            submit(i % 2, views)
        ctx.wait(0)
        ctx.wait(1)
        fps = iters * F / (time.perf_counter() - t0)
        return fps, seen + [read(s) for s in range(min(2, iters))]

    def read_labels(slot):
        return dict(ctx.timing(slot), **ctx.label_timing(slot))

    med = lambda ts, k: float(np.median([t[k] for t in ts]))      # noqa: E731
    out = {"metric": "label_frames_per_s", "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "host_threads": ctx.host_threads,
           "map_objects": scene.mobj_count()}
    loop(ctx.submit_labels, 2, read_labels)                       # warm-up: clocks, code resident, arenas grown, the slots' label buffers
    loop(ctx.submit_depth, 2, ctx.timing)
    rounds = {"label_fps": [], "label_host_ms": [], "label_tiles_ms": [], "label_boxes_ms": [], "depth_tiles_ms": [], "depth_fps": []}
    for _ in range(args.rounds):
        fps, ts = loop(ctx.submit_labels, args.iters, read_labels)
        assert all(t["front_end"] == dg.DG_FE_LABELS for t in ts)
        rounds["label_fps"].append(fps)
        for k, name in (("host_ms", "label_host_ms"), ("tiles_ms", "label_tiles_ms"), ("boxes_ms", "label_boxes_ms")):
            rounds[name].append(med(ts, k))
        fps, ts = loop(ctx.submit_depth, args.iters, ctx.timing)
        assert all(t["front_end"] == dg.DG_FE_DEPTH for t in ts)
        rounds["depth_fps"].append(fps)
        rounds["depth_tiles_ms"].append(med(ts, "raster_ms"))
    m = {k: float(np.median(v)) for k, v in rounds.items()}
    out.update(label_frames_per_s=round(m["label_fps"], 1), depth_frames_per_s=round(m["depth_fps"], 1), label_host_ms=round(m["label_host_ms"], 4),
               label_tiles_ms=round(m["label_tiles_ms"], 4), label_boxes_ms=round(m["label_boxes_ms"], 4), depth_tiles_ms=round(m["depth_tiles_ms"], 4))
    for k in ("label_tiles_ms", "label_boxes_ms", "depth_tiles_ms"):
        out[k + "_rounds"] = [round(v, 4) for v in rounds[k]]
    out["label_tiles_over_depth_tiles"] = round(m["label_tiles_ms"] / m["depth_tiles_ms"], 3)
    out["boxes_read_gb_per_s"] = round(3.0 * W * H * F / (m["label_boxes_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
