#!/usr/bin/env python3
"""plane_reduce_bench.py — frames/s whose depth and label planes reach the host, full size and reduced (dg_readback_planes_reduced_async),
on one MI355X.

    python tools/plane_reduce_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10]

Workload: views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), submitted as bundles of all three parts
(dg_submit_bundle_views) of B = dg_bundle_capacity frames on a ctx of max_batch --batch, round robin over two slots, every outputs' host
memory page-locked.  Prints one JSON line:
  full_frames_per_s        every bundle followed by dg_readback_depth + dg_readback_labels of all its frames: 6 bytes per pixel over
                           PCIe, two blocking calls per bundle — the only route before the reduced readbacks, measured in the same run
  none_frames_per_s        the same loop with no readback at all: what the bundles themselves allow (host list generation + kernels)
  <case>_frames_per_s      the same loop with dg_readback_planes_reduced_async of the four planes (no boxes) queued behind every bundle,
                           <case> = point_2x2, point_4x4, point_8x8, nearest_2x2, nearest_4x4, nearest_8x8
  <case>_speedup           ... over full_frames_per_s
  <case>_kernel_ms_per_1000  median GPU time of the kernel over the B frames of slot 0 (dg_reduce_planes_device, events attached to the
                           dispatch), scaled to 1 000 frames
  d2d_copy_ms_per_1000     median GPU time of a device-to-device hipMemcpyAsync of the B distance planes (2 bytes per pixel: the bytes the
                           NEAREST kernel reads from end to end), in the same run: the yardstick for that kernel
  nearest_*_kernel_over_copy  the ratio of the two
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIP_MEMCPY_D2D = 3
NAMES = ("distance", "kind", "id", "cls")
BYTES = {"distance": 2, "kind": 1, "id": 2, "cls": 1}


def run(args) -> dict:
    import torch
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H = args.width, args.height
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=args.batch, slots=2)
    ctx.upload_scene(scene)
    what = dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH | dg.DG_BUNDLE_LABELS
    B = ctx.bundle_capacity(what)
    if B < 1:
        raise SystemExit(f"a slab of {args.batch} frames holds no bundle of all three parts")
    views = dg.make_views(np.resize(path, (B, 8)))
    n_mobjs = scene.mobj_count()
    L = dg.lib()
    px = W * H
    # page-locked outputs: one full-size set (the full-size calls block, so one is enough), two reduced sets sized for 2x2
    full = {k: L.dg_alloc_host(B * px * BYTES[k]) for k in NAMES}
    full["boxes"] = L.dg_alloc_host(max(1, B * n_mobjs * dg.LABEL_BOX_DTYPE.itemsize))
    ow2, oh2 = dg.plane_reduced_size(W, H, (2, 2))
    small = [{k: L.dg_alloc_host(B * ow2 * oh2 * BYTES[k]) for k in NAMES} for _ in range(2)]
    assert all(full.values()) and all(all(s.values()) for s in small)
    P = ctypes.c_void_p

    def loop(after_submit, iters):
        t0 = time.perf_counter()
        for i in range(iters):
            ctx.submit_bundle(i % 2, views, what)
            after_submit(i % 2)
        ctx.wait(0)
        ctx.wait(1)
        return iters * B / (time.perf_counter() - t0)

    def read_full(s):
        rc = L.dg_readback_depth(ctx._h, s, 0, B, P(full["distance"]), P(full["kind"]))
        rc = rc or L.dg_readback_labels(ctx._h, s, 0, B, P(full["id"]), P(full["cls"]), P(full["boxes"]))
        assert rc == 0, L.dg_last_error()

    cases = {f"{name}_{f}x{f}": (f, f, rule) for name, rule in (("point", dg.DG_PLANE_POINT), ("nearest", dg.DG_PLANE_NEAREST)) for f in (2, 4, 8)}
    out = {"metric": "reduced_planes_frames_per_s", "width": W, "height": H, "batch": args.batch, "frames_per_bundle": B, "iters": args.iters}
    loop(read_full, 2)                                        # warm-up: clocks, code resident, the host buffers touched
    out["full_frames_per_s"] = round(loop(read_full, args.iters), 1)
    out["full_pcie_gb_s"] = round(out["full_frames_per_s"] * 6 * px / 1e9, 2)
    loop(lambda s: None, 2)
    out["none_frames_per_s"] = round(loop(lambda s: None, args.iters), 1)
    for name, d in cases.items():
        reduced = lambda s, d=d: ctx.readback_planes_reduced_async(s, 0, B, d, **small[s])
        loop(reduced, 2)
        fps = loop(reduced, args.iters)
        out[f"{name}_frames_per_s"] = round(fps, 1)
        out[f"{name}_speedup"] = round(fps / out["full_frames_per_s"], 2)

    # the kernel alone over the planes of slot 0, and a device-to-device copy of its distance planes
    ctx.submit_bundle(0, views, what)
    ctx.wait(0)
    lay = dg.bundle_layout(W, H, B, what)
    fb = ctx.framebuffer_ptr(0)
    src = {k: fb + lay[k] for k in NAMES}
    dst_t = {k: torch.empty(B * px * BYTES[k], dtype=torch.uint8, device="cuda") for k in NAMES}
    dst = {k: t.data_ptr() for k, t in dst_t.items()}
    torch.cuda.synchronize()
    for name, d in cases.items():
        ms = []
        for _ in range(args.iters + 1):
            ctx.reduce_planes_device(W, H, B, d, src, dst)
            ms.append(ctx.plane_reduce_kernel_ms())
        out[f"{name}_kernel_ms_per_1000"] = round(float(np.median(ms[1:])) * 1000.0 / B, 4)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    ms = []
    for _ in range(args.iters + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = hip.hipMemcpyAsync(dst["distance"], src["distance"], 2 * B * px, HIP_MEMCPY_D2D, stream.cuda_stream)
        assert rc == 0, rc
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    copy_ms = float(np.median(ms[1:]))
    out["d2d_copy_ms_per_1000"] = round(copy_ms * 1000.0 / B, 4)
    out["d2d_copy_read_tb_s"] = round(2 * B * px / (copy_ms * 1e-3) / 1e12, 3)
    for name in cases:
        if name.startswith("nearest"):
            out[f"{name}_kernel_read_tb_s"] = round(2 * px * 1000 / (out[f"{name}_kernel_ms_per_1000"] * 1e-3) / 1e12, 3)
            out[f"{name}_kernel_over_copy"] = round(out[f"{name}_kernel_ms_per_1000"] / out["d2d_copy_ms_per_1000"], 3)
    for p in list(full.values()) + [p for s in small for p in s.values()]:
        L.dg_free_host(p)
    ctx.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    print(json.dumps(run(args)))


if __name__ == "__main__":
    main()
