#!/usr/bin/env python3
"""overlay_bench.py — dg_slot_overlay's kernel next to the raster launch of the frames it draws on, on one MI355X, in one process.

    python tools/overlay_bench.py [--width 1280 --height 800] [--batch 64] [--iters 10] [--rounds 3]

One slot of --batch frames (a full max_batch) of the seed-1993 path.  The screen: a 320 x 32 status bar at scale 4 along the bottom, a
weapon-sized sprite picture (TROOA1, 43 x 57) at scale 4 with DG_PIC_OFFSETS above it, drawn before the bar, and a 9 x 9 crosshair at
scale 2 at the centre.  Three cases: the screen on every frame, on every eighth frame, and on no frame (nothing is launched: kernel_ms 0,
the call's wall time is what is left).  Per case, after a warm-up, --rounds rounds of --iters calls: the median of
dg_ctx_overlay_kernel_ms (events on the dispatch) per round and over the rounds, the run-to-run spread of the rounds, the call's wall
time, the bytes the kernel stores per batch (three per pixel an item sets, counted with dg_overlay_host) and the GB/s that implies; next
to it raster_ms of the same slot from dg_slot_timing.  Prints one JSON line."""
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    scene = dg.Scene(sw.append_lumps(sw.build_synth_iwad(1993), sw.hud_lumps(1993)), "e1m1")
    weapon, bar, cross = (scene.use_picture(n) for n in ("TROOA1", "STBAR", "XHAIR"))
    screen = [(weapon, W // 2, H - 32 * 4 + 40, 4, 4, 255, dg.DG_PIC_OFFSETS), (bar, 0, H - 32 * 4, 4, 4, 255, 0), (cross, W // 2, H // 2, 2, 2, 255, dg.DG_PIC_OFFSETS)]
    # the pixels one frame's screen sets: those on which a black and a white frame agree afterwards
    two = np.stack([np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)])
    dg.overlay_host(scene, two, [screen, screen])
    stored_px = int((two[0] == two[1]).all(axis=-1).sum())
    ctx = dg.Context(W, H, max_batch=F, slots=1)
    ctx.upload_scene(scene)
    ctx.submit(0, dg.make_views(np.resize(path, (F, 8))))
    ctx.wait(0)
    raster_ms = ctx.timing(0)["raster_ms"]
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "overlay", "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "raster_ms": round(raster_ms, 4),
           "stored_pixels_per_frame": stored_px, "cases": []}
    for name, every in (("every frame", 1), ("every eighth frame", 8), ("no items", 0)):
        lists = [screen if every and f % every == 0 else [] for f in range(F)]
        frames_with = sum(1 for l in lists if l)

        def call():
            t0 = time.perf_counter()
            ctx.slot_overlay(0, 0, lists)
            wall = (time.perf_counter() - t0) * 1e3
            return (ctx.overlay_kernel_ms() if frames_with else 0.0), wall

        for _ in range(2):
            call()
        rk, rw = [], []
        for _ in range(args.rounds):
            r = [call() for _ in range(args.iters)]
            rk.append(med([k for k, _ in r]))
            rw.append(med([w for _, w in r]))
        k = med(rk)
        stored = 3 * stored_px * frames_with
        out["cases"].append({"case": name, "frames_with_items": frames_with, "kernel_ms": round(k, 4), "kernel_ms_rounds": [round(v, 4) for v in rk],
                             "spread_ms": round(max(rk) - min(rk), 4), "call_wall_ms": round(med(rw), 4), "stored_bytes": stored,
                             "stored_gb_s": round(stored / (k * 1e-3) / 1e9, 1) if k > 0 else 0.0, "kernel_over_raster": round(k / raster_ms, 4) if raster_ms > 0 else None})
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
