#!/usr/bin/env python3
"""mobj_pose_bench.py — what per-view map-object poses cost the forced seg walk on one MI355X, in one run.

    python tools/mobj_pose_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), --batch frames per
submission through DG_FE_DEVICE_SEGS, with 0, 1 and all map objects moved per view (each to the position of a later path frame) and, as
the yardstick, the same batch without poses.  Prints one JSON line.  Per round --iters replays of one submission each; medians of
    pose_kernels_ms      dg_mobj_pose_fill + dg_mobj_pose_place (dg_slot_mobj_pose_timing: events on their dispatches)
    front_end_ms         the whole front-end chain (dg_slot_timing setup_ms: the pose kernels, the seg walk, the column walk)
    raster_ms, total_ms  the raster launch and both
for the kinds none (poses == NULL), moved0 (a dg_view_poses array whose n are all 0: the fill kernel alone), moved1 and moved_all.
host_ms is the submission's host time (the entries' de-duplication and staging are in it).  Every kind's fallback counters are printed:
a seg-walk batch with poses must not fall back.
"""
import argparse
import importlib
import json
import os
import sys

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
    recs = np.resize(path, (F, 8))
    views = dg.make_views(recs)
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    n_mobjs = scene.mobj_count()
    ctx = dg.Context(W, H, max_batch=F, slots=1, front_end=dg.DG_FE_DEVICE_SEGS)
    ctx.upload_scene(scene)

    def moved(k):
        """k objects per view, each at the whole-unit position of a later path frame."""
        return [[(m, float(np.rint(path[(f + 3 + 2 * m) % 1000][0])), float(np.rint(path[(f + 3 + 2 * m) % 1000][1])), 0.5 * m) for m in range(k)]
                for f in range(F)]
    kinds = {"none": None, "moved0": moved(0), "moved1": moved(1), "moved_all": moved(n_mobjs)}
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "mobj_poses", "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "map_objects": n_mobjs}
    fields = ("pose_kernels_ms", "front_end_ms", "raster_ms", "total_ms")
    rounds = {k: {f: [] for f in fields} for k in kinds}
    for _ in range(args.rounds):
        for k, entries in kinds.items():
            poses, keep = dg.make_view_poses(entries) if entries is not None else (None, None)
            ctx.submit_poses(0, views, poses)
            ctx.wait(0)
            out[k + "_host_ms"] = round(ctx.timing(0)["host_ms"], 3)
            out[k + "_front_end"] = ctx.timing(0)["front_end"]
            got = {f: [] for f in fields}
            for _ in range(args.iters):
                ctx.replay(0)
                ctx.wait(0)
                t = ctx.timing(0)
                got["pose_kernels_ms"].append(ctx.mobj_pose_timing(0))
                got["front_end_ms"].append(t["setup_ms"])
                got["raster_ms"].append(t["raster_ms"])
                got["total_ms"].append(t["total_ms"])
            for f in fields:
                rounds[k][f].append(med(got[f]))
            out[k + "_fallbacks"] = ctx.fallbacks()
            del keep
    for k in kinds:
        for f in fields:
            out[f"{k}_{f}"] = round(med(rounds[k][f]), 4)
            out[f"{k}_{f}_rounds"] = [round(v, 4) for v in rounds[k][f]]
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
