#!/usr/bin/env python3
"""depth_bench.py — depth frames/s and the time of dg_depth_tiles next to the colour path's kernels on one MI355X.

    python tools/depth_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993) on a ctx created with
DG_FE_HOST, so that the colour path runs from the same host lists the depth path always uses.  Prints one JSON line:
  depth_frames_per_s      frames / wall time of dg_submit_depth_views + dg_wait, --batch frames per submission, two slots round robin
  depth_host_ms           median host list generation of one submission (dg_timing.host_ms): what the rate is expected to be bound by
  depth_tiles_ms          median GPU time of dg_depth_tiles over the --batch frames (the slot's events, attached to the dispatch)
  colour_setup_ms,
  colour_raster_ms        median GPU time of dg_setup_spans and dg_raster_tiles for the SAME views in the same run: the yardstick
  colour_frames_per_s     the same loop with dg_submit_views, for scale
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
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)

    def loop(submit, iters):
        """-> (frames/s, [dg_timing of every submission])"""
        timings = []
        t0 = time.perf_counter()
        for i in range(iters):
            if i >= 2:
                timings.append(ctx.timing(i % 2))             # (waits for the slot, as the next submission into it would)
            submit(i % 2, views)
        ctx.wait(0)
        ctx.wait(1)
        fps = iters * F / (time.perf_counter() - t0)
        return fps, timings + [ctx.timing(s) for s in range(min(2, iters))]

    med = lambda ts, k: round(float(np.median([t[k] for t in ts])), 4)     # noqa: E731
    out = {"metric": "depth_frames_per_s", "width": W, "height": H, "batch": F, "iters": args.iters, "host_threads": ctx.host_threads}
    loop(ctx.submit_depth, 2)                                 # warm-up: clocks, code resident, arenas grown
    fps, ts = loop(ctx.submit_depth, args.iters)
    assert all(t["front_end"] == dg.DG_FE_DEPTH for t in ts)
    out.update(depth_frames_per_s=round(fps, 1), depth_host_ms=med(ts, "host_ms"), depth_tiles_ms=med(ts, "raster_ms"))
    loop(ctx.submit, 2)
    fps, ts = loop(ctx.submit, args.iters)
    assert all(t["front_end"] == dg.DG_FE_HOST for t in ts)
    out.update(colour_frames_per_s=round(fps, 1), colour_host_ms=med(ts, "host_ms"), colour_setup_ms=med(ts, "setup_ms"), colour_raster_ms=med(ts, "raster_ms"))
    out["colour_kernels_ms"] = round(out["colour_setup_ms"] + out["colour_raster_ms"], 4)
    out["depth_over_colour_kernels"] = round(out["depth_tiles_ms"] / out["colour_kernels_ms"], 3)
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
