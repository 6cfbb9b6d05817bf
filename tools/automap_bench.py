#!/usr/bin/env python3
"""automap_bench.py — throughput of the 2-D map view (dg_submit_map_views) on one MI355X.

    python tools/automap_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 30] [--rocprof]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), submitted as batches of
--batch frames round robin over two slots (a slot's next submission waits for its last).  Prints one JSON line:
  frames_per_s       frames / wall time over --iters submissions (host arrow setup + H2D + kernels, pipelined over the slots)
  kernel_ms          median dg_slot_timing raster_ms of --iters replays of one batch (copy + arrow kernels, event-timed)
  write_tb_s         3*W*H*batch bytes / kernel_ms, and fill_share: that rate over the 6.9 TB/s pure fill DESIGN.md records
With --rocprof the same run is repeated as a fresh child under `rocprofv3 --kernel-trace --stats` and the per-kernel averages of the
map kernels are added (rocprof_*_us).
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILL_TB_S = 6.9        # pure-fill rate of one MI355X measured by tools/microbench/hbm_copy.py


def run(args) -> dict:
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    recs = np.resize(path, (F, 8))
    views = dg.make_views(recs)
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(scene)
    ctx.submit_map(0, views)                      # builds the linedef layer
    ctx.wait(0)
    build = ctx.timing(0)
    for i in range(4):                            # warm-up: clocks, code resident
        ctx.submit_map(i % 2, views)
    ctx.wait(0)
    ctx.wait(1)
    t0 = time.perf_counter()
    for i in range(args.iters):
        ctx.submit_map(i % 2, views)
    ctx.wait(0)
    ctx.wait(1)
    wall = time.perf_counter() - t0
    ks = []
    for _ in range(args.iters):
        ctx.replay(0)
        ctx.wait(0)
        ks.append(ctx.timing(0)["raster_ms"])
    kernel_ms = float(np.median(ks))
    tb_s = 3.0 * W * H * F / (kernel_ms * 1e-3) / 1e12
    out = {"metric": "automap_frames_per_s", "width": W, "height": H, "batch": F, "iters": args.iters,
           "frames_per_s": round(args.iters * F / wall, 1), "kernel_ms": round(kernel_ms, 4),
           "kernel_frames_per_s": round(F / (kernel_ms * 1e-3), 1), "write_tb_s": round(tb_s, 3),
           "fill_share": round(tb_s / FILL_TB_S, 3), "layer_build_ms": round(build["setup_ms"], 4)}
    ctx.close()
    scene.close()
    return out


def rocprof(args) -> dict:
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="automap_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--width", str(args.width), "--height", str(args.height), "--batch", str(args.batch), "--iters", str(min(args.iters, 10))]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    res = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                for k in ("dg_map_copy", "dg_map_arrow", "dg_map_layer_steps", "dg_map_layer_resolve"):
                    if k in name:
                        res[f"rocprof_{k}_us"] = round(float(row["AverageNs"]) / 1e3, 2)
                        res[f"rocprof_{k}_calls"] = int(row["Calls"])
    shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rocprof", action="store_true")
    args = ap.parse_args()
    out = run(args)
    if args.rocprof:
        out.update(rocprof(args))
        cp = out.get("rocprof_dg_map_copy_us")
        if cp is not None:
            per_batch = cp + out.get("rocprof_dg_map_arrow_us", 0.0)
            out["rocprof_kernel_ms"] = round(per_batch / 1e3, 4)
            out["rocprof_fill_share"] = round(3.0 * args.width * args.height * args.batch / (per_batch * 1e-6) / 1e12 / FILL_TB_S, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
