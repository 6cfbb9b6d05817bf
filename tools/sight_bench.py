#!/usr/bin/env python3
"""sight_bench.py — what a line-of-sight pass over every (view, map object) pair costs on one MI355X, next to the host twin and to the
frames of the same batch, in one run.

    python tools/sight_bench.py [--width 320 --height 200] [--batch 1000] [--rounds 7] [--synth-map 2002:32x24:500] [--only light|synth]

Workload: --batch views — on the light map (build_synth_iwad(1993)) the views of tests/golden/campath_seed1993.f32, on the generated map
of --synth-map (SEED:COLUMNSxROWS:THINGS, heavy + vanilla, as bench.py builds it) views next to its vertices — and every map object
56 units tall, eye height 41.  Two kinds: "plain" (no entries) and "door" (one dg_view_sectors entry per frame: a sector's floor raised
to its ceiling, another sector each frame).  Prints one JSON line per map.  Per kind, over --rounds rounds that alternate the two
paths (the first round warms up and is not counted), median / min / max of
    device_wall_ms    dg_sight_mobjs_device, wall clock (the call is synchronous: entries, uploads, kernels and the copy back are in it)
    rows_ms, sight_ms dg_ctx_sight_kernel_ms: the row kernels and dg_sight_mobjs, from the events on their dispatches
    host_wall_ms      dg_sight_mobjs_host on the ctx's host threads: the batch cut into one run of frames per thread, each run one call
    host_1_wall_ms    ... and in one call on one thread
and, once, that device and host rows are equal and how many pairs are visible.  render_wall_ms: dg_render_views of the same views at
--width x --height, median of the same rounds — what a step costs before a sight pass is added to it.
"""
import argparse
import importlib
import json
import os
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EYE, TALL = 41.0, 56.0


def vertex_views(dg, sw, scene, wad, n):
    """n views next to the map's vertices, spread over the lump, each on the floor it stands on."""
    d = sw.wad_directory(wad)
    i = next(k for k, (name, _, _) in enumerate(d) if name == "E1M1")
    _, off, size = d[i + 4]
    verts = list(struct.iter_unpack("<hh", wad[off:off + size - size % 4]))
    arr = (dg.DgView * n)()
    for k in range(n):
        x, y = verts[(k * 7919) % len(verts)]
        x, y = float(x) + 3.5, float(y) - 2.25
        arr[k] = dg.DgView(x, y, 0.1 * k, scene.floor_height_at(x, y), 0, 0, 0, 0, 0.1 * k, 0)
    return arr


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def measure(dg, name, wad, make_views, args):
    F = args.batch
    scene = dg.Scene(wad, "e1m1")
    views = make_views(scene, wad)
    n_obj, n_sec = scene.mobj_count(), len(scene.sector_heights())
    heights = np.full(n_obj, TALL, dtype=np.float32)
    ctx = dg.Context(args.width, args.height, max_batch=F, slots=1)
    ctx.upload_scene(scene)
    threads = max(1, ctx.host_threads)
    pool = ThreadPoolExecutor(threads)
    sec = scene.sector_heights()
    doors = [[(f % n_sec, int(sec[f % n_sec][1]), int(sec[f % n_sec][1]))] for f in range(F)]
    door_arr, keep = dg.make_view_sectors(doors)
    cuts = [(F * t // threads, F * (t + 1) // threads) for t in range(threads)]
    runs = []                                                  # per thread: its views, and its entries as an array of its own
    for a, b in cuts:
        part, keep_part = dg.make_view_sectors(doors[a:b])
        runs.append(((dg.DgView * (b - a))(*[views[i] for i in range(a, b)]), part, keep_part))

    def host_threads(sectors_on):
        parts = list(pool.map(lambda r: dg.sight_mobjs_host(scene, r[0], EYE, heights, None, r[1] if sectors_on else None), [r for r in runs if len(r[0])]))
        return np.concatenate(parts)

    out = {"metric": "sight_mobjs", "map": name, "batch": F, "map_objects": n_obj, "sectors": n_sec, "bsp_depth": scene.bsp_depth(), "host_threads": threads,
           "rounds": args.rounds, "render_size": [args.width, args.height]}
    render = []
    for kind, sectors in (("plain", None), ("door", door_arr)):
        t = {k: [] for k in ("device_wall_ms", "rows_ms", "sight_ms", "host_wall_ms", "host_1_wall_ms")}
        for r in range(args.rounds + 1):
            d_ms, dev = wall_ms(lambda: ctx.sight_mobjs(views, EYE, heights, None, sectors))
            k_ms = ctx.sight_kernel_ms()
            h_ms, host = wall_ms(lambda: host_threads(sectors is not None))
            h1_ms, host1 = wall_ms(lambda: dg.sight_mobjs_host(scene, views, EYE, heights, None, sectors))
            r_ms, _ = wall_ms(lambda: ctx.render(views))
            if r == 0:                                         # warm-up: code objects, first-use allocations, the page cache of the outputs
                if not (np.array_equal(dev, host) and np.array_equal(dev, host1)):
                    raise SystemExit(f"{name} {kind}: device and host rows differ")
                out[kind + "_visible_pairs"] = int(sum(bin(int(w)).count("1") for w in dev.ravel()))
                continue
            for key, v in (("device_wall_ms", d_ms), ("rows_ms", k_ms["rows_ms"]), ("sight_ms", k_ms["sight_ms"]), ("host_wall_ms", h_ms), ("host_1_wall_ms", h1_ms)):
                t[key].append(v)
            render.append(r_ms)
        out[kind] = {k: spread(v) for k, v in t.items()}
        out[kind]["host_over_device"] = round(float(np.median(t["host_wall_ms"]) / np.median(t["device_wall_ms"])), 2)
    out["render_wall_ms"] = spread(render)
    del keep
    pool.shutdown()
    ctx.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--synth-map", default="2002:32x24:500")
    ap.add_argument("--only", choices=["light", "synth"], default=None)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    if args.only != "synth":
        path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
        print(json.dumps(measure(dg, "light (seed 1993)", sw.build_synth_iwad(1993), lambda scene, wad: dg.make_views(np.resize(path, (args.batch, 8))), args)), flush=True)
    if args.only != "light":
        seed, grid, things = args.synth_map.split(":")
        wad = sw.build_synth_iwad(int(seed), heavy=True, vanilla=True, grid=tuple(int(v) for v in grid.split("x")), n_things=int(things))
        print(json.dumps(measure(dg, f"synth {args.synth_map}", wad, lambda scene, w: vertex_views(dg, sw, scene, w, args.batch), args)), flush=True)


if __name__ == "__main__":
    main()
