#!/usr/bin/env python3
"""observe_bench.py — dg_observe_device next to the route it replaces, on one MI355X, in one process.

    python tools/observe_bench.py [--width 1280 --height 800] [--batch 256] [--iters 10] [--rounds 3]

Source: one bundle slot (colour + depth) of --batch frames of the seed-1993 path, resident in device memory.
Configurations: source in {RGB, GRAY, DISTANCE/NEAREST} x box in {1x1, 4x4, 8x8} x dtype in {F16, F32}, contiguous NCHW; maps 1/255 for
colour, 1/2048 with hi = 2048 for distance.  Per configuration, after a warm-up of both routes, --rounds interleaved rounds of --iters
calls each, medians of
  (a) observe_ms   dg_ctx_observe_kernel_ms (events on the dispatch);
  (b) route_ms     today's route into a preallocated output: dg_reduce_device / dg_reduce_planes_device (its kernel ms) plus the torch
                   chain behind it — clamp_ (distance), copy_ of the permuted view (permute + .to(dtype) in one kernel), mul_ (and add_
                   when the bias is not 0) — between two torch events on torch's stream.
Prints one JSON line: per configuration both medians, the per-round medians, route_ms / observe_ms, `wins` (route_ms - observe_ms above
the larger spread of the rounds) and (a)'s bytes read + written per second; and hbm_copy_gb_s, a device-to-device copy of 768 MiB
(tools/microbench/hbm_copy.py's measurement) in the same process."""
import torch  # noqa: E402  (before libdoomgpu.so is loaded: INTEGRATION.md)

import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hbm_copy_gb_s():
    n = 768 * 1024 * 1024
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2 * n / (e0.elapsed_time(e1) / 20) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    what = dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=3 * F, slots=1)
    ctx.upload_scene(scene)
    ctx.submit_bundle(0, dg.make_views(np.resize(path, (F, 8))), what)
    ctx.wait(0)
    lay = dg.bundle_layout(W, H, F, what)
    fb = ctx.framebuffer_ptr(0)
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "observe", "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "configs": []}
    tdt = {dg.DG_OBS_F16: torch.float16, dg.DG_OBS_F32: torch.float32}
    for source, name in ((dg.DG_OBS_RGB, "rgb"), (dg.DG_OBS_GRAY, "gray"), (dg.DG_OBS_DISTANCE, "distance_nearest")):
        colour = source != dg.DG_OBS_DISTANCE
        src = fb + (lay["colour"] if colour else lay["distance"])
        scale, lo, hi = (float(np.float32(1) / np.float32(255)), -32768, 32767) if colour else (1.0 / 2048.0, -32768, 2048)
        for f in (1, 4, 8):
            for dtype in (dg.DG_OBS_F16, dg.DG_OBS_F32):
                d = dg.DgObsDesc(f, f, source, dg.DG_PLANE_NEAREST if not colour else 0, dtype, lo, hi, scale, 0.0, 0)
                C, oH, oW, eb = dg.observed_size(W, H, d)
                obs = torch.empty((F, C, oH, oW), dtype=tdt[dtype], device="cuda")
                ref = torch.empty_like(obs)
                if colour:
                    red = torch.empty((F, oH, oW, 3) if source == dg.DG_OBS_RGB else (F, oH, oW, 1), dtype=torch.uint8, device="cuda")
                    rdesc = (f, f, dg.DG_REDUCE_RGB24 if source == dg.DG_OBS_RGB else dg.DG_REDUCE_GRAY8)
                else:
                    red = torch.empty((F, oH, oW, 1), dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def route_a():
                    ctx.observe_into(src, W, H, F, d, obs)
                    return ctx.observe_kernel_ms()

                def route_b():
                    if colour:
                        ctx.reduce_device(src, W, H, F, rdesc, red.data_ptr())
                        k = ctx.reduce_kernel_ms()
                    else:
                        ctx.reduce_planes_device(W, H, F, (f, f, dg.DG_PLANE_NEAREST), {"distance": src}, {"distance": red.data_ptr()})
                        k = ctx.plane_reduce_kernel_ms()
                    e0.record()
                    if not colour:
                        red.clamp_(max=hi)
                    ref.copy_(red.permute(0, 3, 1, 2))
                    ref.mul_(scale)
                    e1.record()
                    torch.cuda.synchronize()
                    return k, e0.elapsed_time(e1)

                for _ in range(2):                             # warm-up of every shape the timed window uses
                    route_a()
                    route_b()
                # the two routes compute the same tensor up to the route's own rounding (it multiplies in the narrow type)
                err = float((obs.float() - ref.float()).abs().max())
                assert err <= 2e-3, (name, f, dtype, err)
                ra, rb, rk = [], [], []
                for _ in range(args.rounds):
                    ra.append(med([route_a() for _ in range(args.iters)]))
                    kb = [route_b() for _ in range(args.iters)]
                    rb.append(med([k + t for k, t in kb]))
                    rk.append(med([k for k, _ in kb]))
                a, b = med(ra), med(rb)
                spread = max(max(ra) - min(ra), max(rb) - min(rb))
                moved = F * W * H * (3 if colour else 2) + F * C * oH * oW * eb
                out["configs"].append({"source": name, "box": f, "dtype": dg.OBS_DTYPE_NAMES[dtype], "observe_ms": round(a, 4), "route_ms": round(b, 4),
                                       "route_reduce_kernel_ms": round(med(rk), 4), "observe_ms_rounds": [round(v, 4) for v in ra],
                                       "route_ms_rounds": [round(v, 4) for v in rb], "route_over_observe": round(b / a, 3), "spread_ms": round(spread, 4),
                                       "wins": bool(b - a > spread), "observe_gb_s": round(moved / (a * 1e-3) / 1e9, 1), "max_abs_diff": err})
                del obs, ref, red
    out["hbm_copy_gb_s"] = round(hbm_copy_gb_s(), 1)
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
