#!/usr/bin/env python3
"""reduce_bench.py — frames/s delivered to the host with and without the box downscale (dg_readback_reduced_async) on one MI355X.

    python tools/reduce_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rocprof]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), submitted as batches of
--batch frames round robin over two slots, every batch followed by an asynchronous readback into page-locked host memory (a slot's next
submission completes its last readback).  Prints one JSON line:
  plain_frames_per_s      frames / wall time with dg_readback_async: the whole frames over PCIe, the baseline
  <case>_frames_per_s     the same loop with dg_readback_reduced_async, <case> = rgb_2x2, rgb_4x4, rgb_8x8, gray_4x4
  <case>_speedup          ... over plain_frames_per_s
  <case>_kernel_ms        median GPU time of dg_reduce over the --batch frames of slot 0 (dg_reduce_device, events attached to the dispatch)
  d2d_copy_ms             median GPU time of a device-to-device hipMemcpyAsync of the same --batch source frames, in the same run: the
                          yardstick for the kernel (it reads the same bytes and writes at most a quarter as many)
With --rocprof the same run is repeated as a fresh child under `rocprofv3 --kernel-trace --stats` and the per-kernel averages of
dg_reduce are added (rocprof_*_us).
"""
import argparse
import csv
import ctypes
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
HIP_MEMCPY_D2D = 3


def run(args) -> dict:
    import torch
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(scene)
    bufs = [dg.lib().dg_alloc_host(F * ctx.frame_bytes) for _ in range(2)]
    assert all(bufs)
    cases = {"rgb_2x2": (2, 2, dg.DG_REDUCE_RGB24), "rgb_4x4": (4, 4, dg.DG_REDUCE_RGB24), "rgb_8x8": (8, 8, dg.DG_REDUCE_RGB24),
             "gray_4x4": (4, 4, dg.DG_REDUCE_GRAY8)}

    def loop(readback, iters):
        t0 = time.perf_counter()
        for i in range(iters):
            ctx.submit(i % 2, views)
            readback(i % 2)
        ctx.wait(0)
        ctx.wait(1)
        return iters * F / (time.perf_counter() - t0)

    out = {"metric": "reduced_readback_frames_per_s", "width": W, "height": H, "batch": F, "iters": args.iters}
    plain = lambda s: ctx.readback_async(s, 0, F, bufs[s])
    loop(plain, 2)                                            # warm-up: clocks, code resident, the host buffers touched
    out["plain_frames_per_s"] = round(loop(plain, args.iters), 1)
    out["plain_pcie_gb_s"] = round(out["plain_frames_per_s"] * ctx.frame_bytes / 1e9, 2)
    for name, d in cases.items():
        reduced = lambda s, d=d: ctx.readback_reduced_async(s, 0, F, d, bufs[s])
        loop(reduced, 2)
        fps = loop(reduced, args.iters)
        out[f"{name}_frames_per_s"] = round(fps, 1)
        out[f"{name}_speedup"] = round(fps / out["plain_frames_per_s"], 2)

    # the kernel alone over the frames of slot 0, and a device-to-device copy of the same frames
    src = ctx.framebuffer_ptr(0)
    dst = torch.empty(F * ctx.frame_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for name, d in cases.items():
        ms = []
        for _ in range(args.iters + 1):
            ctx.reduce_device(src, W, H, F, d, dst.data_ptr())
            ms.append(ctx.reduce_kernel_ms())
        k = float(np.median(ms[1:]))
        out[f"{name}_kernel_ms"] = round(k, 4)
        out[f"{name}_kernel_read_tb_s"] = round(F * ctx.frame_bytes / (k * 1e-3) / 1e12, 3)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    ms = []
    for _ in range(args.iters + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src, F * ctx.frame_bytes, HIP_MEMCPY_D2D, stream.cuda_stream)
        assert rc == 0, rc
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out["d2d_copy_ms"] = round(float(np.median(ms[1:])), 4)
    out["d2d_copy_read_tb_s"] = round(F * ctx.frame_bytes / (out["d2d_copy_ms"] * 1e-3) / 1e12, 3)
    for name in cases:
        out[f"{name}_kernel_over_copy"] = round(out[f"{name}_kernel_ms"] / out["d2d_copy_ms"], 3)
    for b in bufs:
        dg.lib().dg_free_host(b)
    ctx.close()
    scene.close()
    return out


def rocprof(args) -> dict:
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="reduce_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--width", str(args.width), "--height", str(args.height), "--batch", str(args.batch), "--iters", str(min(args.iters, 4))]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    res = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "dg_reduce" in row.get("Name", ""):
                    key = "rocprof_dg_reduce_pieces" if "true" in row["Name"] or "Lb1" in row["Name"] else "rocprof_dg_reduce_anyw"
                    res[f"{key}_us"] = round(float(row["AverageNs"]) / 1e3, 2)
                    res[f"{key}_calls"] = int(row["Calls"])
    shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    args = ap.parse_args()
    out = run(args)
    if args.rocprof:
        out.update(rocprof(args))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
