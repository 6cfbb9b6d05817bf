#!/usr/bin/env python3
"""walk_bench.py — locating the floors of recorded walks: the host path against dg_ctx_locate_walks on one MI355X.

    python tools/walk_bench.py [--walks 256] [--tics 21000] [--seed 7] [--synth-map 2002:32x24:500] [--only light|synth]

Workload: --walks walks of --tics tics each (21 000 tics = ten minutes of play) from Player1Start with seeded random key masks, on the
light map (build_synth_iwad(1993)) and on the doom2-scale generated map of --synth-map (SEED:COLUMNSxROWS:THINGS, heavy + vanilla, as
bench.py builds it).  For each map it creates the walks twice and reports, in one JSON line per map:
  create_ms       dg_walk_create of all walks (the serial pose integration with libm; the same on either side)
  host_ms         dg_walk_floors on every walk of the first set: one BSP descent per probe on the host, one walk after the other
  gpu_ms          dg_ctx_locate_walks on the second set, transfers included; gpu_first_ms is the first call (it also uploads the node
                  and leaf tables and creates the stream), gpu_ms the median of the calls on fresh walks after it
  equal           the two sets' floors are the same bits
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


def make_walks(dg, scene, keys):
    return [dg.Walk(scene, k) for k in keys]


def measure(dg, name, wad, args) -> dict:
    scene = dg.Scene(wad, "E1M1")
    rng = np.random.default_rng(args.seed)
    keys = [rng.integers(0, 64, args.tics).astype(np.uint8) for _ in range(args.walks)]
    t0 = time.perf_counter()
    host = make_walks(dg, scene, keys)
    create_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host_floors = [w.floors() for w in host]
    host_ms = (time.perf_counter() - t0) * 1e3
    ctx = dg.Context(320, 200, max_batch=1, slots=1)
    ctx.upload_scene(scene)
    gpu_ms, equal = [], True
    for _ in range(args.iters + 1):
        walks = make_walks(dg, scene, keys)
        t0 = time.perf_counter()
        ctx.locate_walks(walks)
        gpu_ms.append((time.perf_counter() - t0) * 1e3)
        equal = equal and all(np.array_equal(w.floors().view(np.uint32), f.view(np.uint32)) for w, f in zip(walks, host_floors))
        for w in walks:
            w.close()
    probes = sum(w.probe_count() for w in host)
    out = {"map": name, "walks": args.walks, "tics": args.tics, "probes": probes, "create_ms": round(create_ms, 2),
           "host_ms": round(host_ms, 2), "gpu_first_ms": round(gpu_ms[0], 2), "gpu_ms": round(float(np.median(gpu_ms[1:])), 2),
           "gpu_ms_min": round(min(gpu_ms[1:]), 2), "gpu_ms_max": round(max(gpu_ms[1:]), 2),
           "host_ns_per_probe": round(host_ms * 1e6 / probes, 1), "equal": bool(equal)}
    for w in host:
        w.close()
    ctx.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=256)
    ap.add_argument("--tics", type=int, default=21000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--synth-map", default="2002:32x24:500")
    ap.add_argument("--only", choices=["light", "synth"], default=None)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    if args.only != "synth":
        print(json.dumps(measure(dg, "light (seed 1993)", sw.build_synth_iwad(1993), args)), flush=True)
    if args.only != "light":
        seed, grid, things = args.synth_map.split(":")
        wad = sw.build_synth_iwad(int(seed), heavy=True, vanilla=True, grid=tuple(int(v) for v in grid.split("x")), n_things=int(things))
        print(json.dumps(measure(dg, f"synth {args.synth_map}", wad, args)), flush=True)


if __name__ == "__main__":
    main()
