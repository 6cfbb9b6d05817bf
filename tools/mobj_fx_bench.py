#!/usr/bin/env python3
"""mobj_fx_bench.py — cost of the map-object state machine (dg_scene_set_mobj_thinkers) on one MI355X.

    python tools/mobj_fx_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 20] [--lights]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32, each at its own timestamp (0 .. 40 s: some 1 400 tics, with a kill at
10 s, a respawn at 20 s and an explode at 30 s), over the test WAD and the hand-written state tables of tests/mobj_fx.py
(build_synth_iwad(1993) plus sprite frames B .. D), submitted as batches of --batch frames round robin over two slots.  --lights turns
the sector light effects on in every configuration (the WAD then also has tests/light_fx.py's sectors), so that a kernel trace of this
run shows dg_light_rows beside dg_mobj_rows.  For each front end (DG_FE_DEVICE, DG_FE_DEVICE_SEGS) and flags 0 and 1
(DG_MOBJ_THINKERS) it reports:
  frames_per_s       frames / wall time over --iters submissions (pipelined over the slots)
  setup_ms, raster_ms  medians of dg_slot_timing over --iters replays of one prepared batch (event-timed kernels: the front-end half —
                     the seg walk, if any, plus the column walk — and the rasteriser)
and, per front end, the change from flags 0 to 1 (part of any raster change is content: other sprite frames are drawn).  Prints one
JSON line.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(dg, scene, views, W, H, F, fe, iters) -> dict:
    ctx = dg.Context(W, H, max_batch=F, slots=2, front_end=fe)
    ctx.upload_scene(scene)
    for i in range(4):                            # warm-up: clocks, code resident, DG_FE_AUTO-free (the front end is forced)
        ctx.submit(i % 2, views)
    ctx.wait(0)
    ctx.wait(1)
    t0 = time.perf_counter()
    for i in range(iters):
        ctx.submit(i % 2, views)
    ctx.wait(0)
    ctx.wait(1)
    wall = time.perf_counter() - t0
    ctx.prepare(0, views)
    setup, raster = [], []
    for _ in range(iters):
        ctx.replay(0)
        ctx.wait(0)
        t = ctx.timing(0)
        setup.append(t["setup_ms"])
        raster.append(t["raster_ms"])
    out = {"frames_per_s": round(iters * F / wall, 1), "setup_ms": round(float(np.median(setup)), 4),
           "raster_ms": round(float(np.median(raster)), 4), "front_end_used": ctx.timing(0)["front_end"],
           "fallbacks": ctx.fallbacks()["front_end"]}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lights", action="store_true")
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    import light_fx
    import mobj_fx
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    F = args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    for k in range(F):
        views[k].timestamp = float(np.float32(40.0 * k / F))
    wad = mobj_fx.fx_wad(light_fx.fx_wad() if args.lights else None)
    res = {"metric": "mobj_fx", "lights": bool(args.lights), "width": args.width, "height": args.height, "batch": F, "iters": args.iters}
    for fe, name in ((2, "device"), (3, "device_segs")):
        for flags in (0, 1):
            scene = dg.Scene(wad, "E1M1")
            if args.lights:
                scene.set_light_effects(dg.DG_LIGHT_THINKERS, 1993)
            scene.set_mobj_thinkers(flags, mobj_fx.STATES, mobj_fx.INFOS)
            if flags:
                for what, t in ((dg.DG_MOBJ_KILL, 10.0), (dg.DG_MOBJ_RESPAWN, 20.0), (dg.DG_MOBJ_EXPLODE, 30.0)):
                    scene.mobj_event(what, t)
            res[f"{name}_flags{flags}"] = measure(dg, scene, views, args.width, args.height, F, fe, args.iters)
            scene.close()
        a, b = res[f"{name}_flags0"], res[f"{name}_flags1"]
        res[f"{name}_fps_change_pct"] = round(100.0 * (b["frames_per_s"] / a["frames_per_s"] - 1.0), 2)
        res[f"{name}_setup_change_pct"] = round(100.0 * (b["setup_ms"] / a["setup_ms"] - 1.0), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
