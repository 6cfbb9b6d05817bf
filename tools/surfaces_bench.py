#!/usr/bin/env python3
"""surfaces_bench.py — what per-view surfaces cost the forced seg walk on one MI355X, in one run.

    python tools/surfaces_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3] [--maps small,large]

Workloads: `small`, the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), and `large`, the
generated map 2002:32x24:500 (doom2's scale) along its own route; --batch frames per submission through DG_FE_DEVICE_SEGS.  Kinds,
interleaved within every round:
    none    surfaces == NULL and sectors == NULL: the plain seg-walk pair, no row kernel (the yardstick)
    hts0    a dg_view_sectors array whose n are all 0: the height fill and the row-reading pair dg_hts_* on the frames of `none`
    same0   a dg_view_surfaces array whose counts are all 0: both fills and the surface-reading pair dg_sfc_* on the frames of `none` —
            against hts0, the difference is what the flat rows and the (empty) sidedef search cost
    switch  one sidedef entry per frame (a switch flipped: its textures rotated)
    flats   an entry for every sector of every frame
    sides   64 sidedef entries per frame: the side table at its capacity, every surviving seg searching a span of 64
Per round --iters replays of one submission each; medians of
    row_kernels_ms       the height row kernels plus the flat row kernels (dg_slot_sector_height_timing + dg_slot_surface_timing)
    front_end_ms         the whole front-end chain (dg_slot_timing setup_ms: the row kernels, the seg walk, the column walk)
    walk_ms              front_end_ms - row_kernels_ms: the seg-walk pair and the column walk behind it
    raster_ms, total_ms  the raster launch and both
gpu_views_per_s is batch / total_ms.  host_ms is the submission's host time (resolving and staging the entries is in it).  Every kind's
fallback counters are printed: a seg-walk batch with surfaces within the side table must not fall back.  Prints one JSON line per map.
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
        sides, flats = scene.sidedef_surfaces(), scene.sector_flats()
        n_sd, n = len(sides), len(flats)
        handles = sorted({int(h) for h in flats[:, 1:].ravel()})
        ctx = dg.Context(W, H, max_batch=F, slots=1, front_end=dg.DG_FE_DEVICE_SEGS)
        ctx.upload_scene(scene)

        def turned(i, by):
            r = sides[i % n_sd]
            return (int(r[0]), int(r[2 if r[2] >= 0 else 1]) if r[1] >= 0 else -1, int(r[3 if r[3] >= 0 else 2]) if r[2] >= 0 else -1,
                    int(r[1 if r[1] >= 0 else 3]) if r[3] >= 0 else -1, int(r[4]) + by, int(r[5]))
        switch = [([turned(37 * f, 1)], []) for f in range(F)]
        one_row = [(s, handles[(s + 1) % len(handles)], handles[(s + 2) % len(handles)]) for s in range(n)]
        full = [([turned(f + 13 * j, j) for j in range(64)], []) for f in range(F)]
        kinds = {"none": ("none", None), "hts0": ("sectors", [[] for _ in range(F)]), "same0": ("surfaces", [([], []) for _ in range(F)]), "switch": ("surfaces", switch),
                 "flats": ("surfaces", [([], one_row)] * F), "sides": ("surfaces", full)}
        out = {"metric": "surfaces", "map": which, "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "sectors": n, "sidedefs": n_sd}
        fields = ("row_kernels_ms", "front_end_ms", "walk_ms", "raster_ms", "total_ms")
        rounds = {k: {f: [] for f in fields} for k in kinds}
        made = {k: (dg.make_view_sectors(e) if how == "sectors" else dg.make_view_surfaces(e) if how == "surfaces" else (None, None)) for k, (how, e) in kinds.items()}
        for _ in range(args.rounds):
            for k, (how, _e) in kinds.items():
                if how == "sectors":
                    ctx.submit_sectors(0, views, made[k][0])
                else:
                    ctx.submit_surfaces(0, views, made[k][0])
                ctx.wait(0)
                out[k + "_host_ms"] = round(ctx.timing(0)["host_ms"], 3)
                out[k + "_front_end"] = ctx.timing(0)["front_end"]
                got = {f: [] for f in fields}
                for _ in range(args.iters):
                    ctx.replay(0)
                    ctx.wait(0)
                    t = ctx.timing(0)
                    rows_ms = ctx.sector_height_timing(0) + ctx.surface_timing(0)
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
