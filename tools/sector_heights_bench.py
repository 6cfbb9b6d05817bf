#!/usr/bin/env python3
"""sector_heights_bench.py — what per-view sector heights cost the forced seg walk on one MI355X, in one run.

    python tools/sector_heights_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3] [--maps small,large]

Workloads: `small`, the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993, 105 sectors), and
`large`, the generated map 2002:32x24:500 (doom2's scale) along its own route; --batch frames per submission through
DG_FE_DEVICE_SEGS.  Kinds, interleaved within every round:
    none   sectors == NULL: the plain seg-walk pair, neither row kernel (the yardstick)
    same0  a dg_view_sectors array whose n are all 0: the fill kernel alone and the row-reading pair over rows equal to the loaded
           heights — the same frames as `none`, so the difference is what reading rows costs
    door   one entry per frame (a door: its ceiling half way up)
    all    an entry for every sector of every frame (jittered heights)
Per round --iters replays of one submission each; medians of
    row_kernels_ms       dg_sector_row_fill + dg_sector_row_scatter (dg_slot_sector_height_timing: events on their dispatches)
    front_end_ms         the whole front-end chain (dg_slot_timing setup_ms: the row kernels, the seg walk, the column walk)
    walk_ms              front_end_ms - row_kernels_ms: the seg-walk pair and the column walk behind it
    raster_ms, total_ms  the raster launch and both
gpu_views_per_s is batch / total_ms.  host_ms is the submission's host time (the entries' de-duplication and staging are in it).  Every
kind's fallback counters are printed: a seg-walk batch with sector entries must not fall back.  Prints one JSON line per map.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(dg, sw, cp, which):
    if which == "small":
        path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
        return dg.Scene(sw.build_synth_iwad(1993), "e1m1"), path
    kw = dict(heavy=True, vanilla=True, grid=(32, 24), n_things=500)
    scene = dg.Scene(sw.build_synth_iwad(2002, **kw), "e1m1")
    return scene, cp.make_camera_path(sw.synth_route(2002, **kw), lambda x, y, d: scene.floor_height_at(x, y, d), 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--maps", default="small,large")
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    cp = importlib.import_module("doom-rust-renderer_amd.camera_path")
    W, H, F = args.width, args.height, args.batch
    med = lambda v: float(np.median(v))                       # noqa: E731
    for which in args.maps.split(","):
        scene, path = workload(dg, sw, cp, which)
        views = dg.make_views(np.resize(path, (F, 8)))
        hs = scene.sector_heights().astype(int)
        n = len(hs)
        ctx = dg.Context(W, H, max_batch=F, slots=1, front_end=dg.DG_FE_DEVICE_SEGS)
        ctx.upload_scene(scene)
        door = [[((7 * f) % n, hs[(7 * f) % n, 0], hs[(7 * f) % n, 0] + (hs[(7 * f) % n, 1] - hs[(7 * f) % n, 0]) // 2)] for f in range(F)]
        one_row = [(s, hs[s, 0] + (7 * s) % 17 - 8, max(hs[s, 1] - (5 * s) % 13, hs[s, 0] + (7 * s) % 17 - 8)) for s in range(n)]
        kinds = {"none": None, "same0": [[] for _ in range(F)], "door": door, "all": [one_row] * F}
        out = {"metric": "sector_heights", "map": which, "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "sectors": n}
        fields = ("row_kernels_ms", "front_end_ms", "walk_ms", "raster_ms", "total_ms")
        rounds = {k: {f: [] for f in fields} for k in kinds}
        made = {k: (dg.make_view_sectors(e) if e is not None else (None, None)) for k, e in kinds.items()}
        for _ in range(args.rounds):
            for k in kinds:
                ctx.submit_sectors(0, views, made[k][0])
                ctx.wait(0)
                out[k + "_host_ms"] = round(ctx.timing(0)["host_ms"], 3)
                out[k + "_front_end"] = ctx.timing(0)["front_end"]
                got = {f: [] for f in fields}
                for _ in range(args.iters):
                    ctx.replay(0)
                    ctx.wait(0)
                    t = ctx.timing(0)
                    rows_ms = ctx.sector_height_timing(0)
                    got["row_kernels_ms"].append(rows_ms)
                    got["front_end_ms"].append(t["setup_ms"])
                    got["walk_ms"].append(t["setup_ms"] - rows_ms)
                    got["raster_ms"].append(t["raster_ms"])
                    got["total_ms"].append(t["total_ms"])
                for f in fields:
                    rounds[k][f].append(med(got[f]))
                out[k + "_fallbacks"] = ctx.fallbacks()
        for k in kinds:
            for f in fields:
                out[f"{k}_{f}"] = round(med(rounds[k][f]), 4)
                out[f"{k}_{f}_rounds"] = [round(v, 4) for v in rounds[k][f]]
            out[f"{k}_gpu_views_per_s"] = round(F / (med(rounds[k]["total_ms"]) * 1e-3), 1)
        print(json.dumps(out), flush=True)
        ctx.close()
        scene.close()


if __name__ == "__main__":
    main()
