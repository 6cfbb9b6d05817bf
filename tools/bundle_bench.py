#!/usr/bin/env python3
"""bundle_bench.py — colour, depth and labels of the same views as ONE bundle submission against three separate submissions, on one MI355X.

    python tools/bundle_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3]

Workload: views of tests/golden/campath_seed1993.f32 (spread evenly over the path) over the synthetic e1m1-like map (seed 1993), a ctx with
DG_FE_HOST, max_batch --batch and two slots.  Every submission — the separate ones too — carries B = dg_bundle_capacity(all three parts)
views, so the comparison is like for like.  The four kinds are measured in alternating rounds (bundle, colour, depth, labels, bundle, ...):
the spread between the rounds of one kind can then be held against the difference between the kinds.  A round is --iters submissions, two
slots round robin; its time per submission is the round's wall time (submit + wait) over --iters.  Prints one JSON line:
  views_per_submission       B
  bundle_views_per_s         B over the bundle's time per submission                       (median of the rounds; *_rounds: each round)
  separate_views_per_s       B over the SUM of the colour, depth and label times per submission of the same round
  bundle_over_separate       the ratio of the two medians
  bundle_faster_beyond_spread   the slowest bundle round beats the fastest separate round
  *_host_ms                  median host list generation + packing of one submission of each kind (dg_timing.host_ms)
  bundle_tiles_ms            median GPU time of dg_bundle_tiles (dg_slot_bundle_timing), next to the kernels it replaces for the same views:
  depth_tiles_ms, label_tiles_ms, label_boxes_ms       (dg_slot_timing of a depth submission, dg_slot_label_timing)
  setup_ms, raster_ms        the colour kernels of the colour submission; bundle_setup_ms, bundle_raster_ms: the same kernels inside the bundle
  tiles_over_replaced        bundle_tiles_ms / (depth_tiles_ms + label_tiles_ms + label_boxes_ms); tiles_below_replaced_beyond_spread: the
                             slowest round of the former is below the smallest round sum of the latter
  tiles_over_depth_plus_label_tiles, tiles_below_depth_plus_label_tiles_beyond_spread   likewise without dg_label_boxes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H = args.width, args.height
    ALL = dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH | dg.DG_BUNDLE_LABELS
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=args.batch, slots=2, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)
    B = ctx.bundle_capacity(ALL)
    if B < 1:
        raise SystemExit(f"a slab of {args.batch} frames holds no bundle of all three parts")
    views = dg.make_views(path[(np.arange(B) * 1000) // B])

    def loop(submit, iters, read):
        """-> (seconds per submission, [what read(slot) gives for every submission])"""
        seen = []
        t0 = time.perf_counter()
        for i in range(iters):
            if i >= 2:
                seen.append(read(i % 2))                       # (waits for the slot, as the next submission into it would)
            submit(i % 2, views)
        ctx.wait(0)
        ctx.wait(1)
        dt = (time.perf_counter() - t0) / iters
        return dt, seen + [read(s) for s in range(min(2, iters))]

    kinds = {
        "bundle": (lambda slot, v: ctx.submit_bundle(slot, v, ALL), lambda slot: dict(ctx.timing(slot), **{"bundle_" + k: t for k, t in ctx.bundle_timing(slot).items()}), dg.DG_FE_BUNDLE),
        "colour": (ctx.submit, ctx.timing, dg.DG_FE_HOST),
        "depth": (ctx.submit_depth, ctx.timing, dg.DG_FE_DEPTH),
        "label": (ctx.submit_labels, lambda slot: dict(ctx.timing(slot), **ctx.label_timing(slot)), dg.DG_FE_LABELS),
    }
    for submit, read, _fe in kinds.values():                      # warm-up: clocks, code resident, arenas grown, the slots' label buffers
        loop(submit, 2, read)
    med = lambda ts, k: float(np.median([t[k] for t in ts]))      # noqa: E731
    names = ("bundle_s", "colour_s", "depth_s", "label_s", "bundle_host_ms", "colour_host_ms", "depth_host_ms", "label_host_ms", "bundle_tiles_ms",
             "bundle_setup_ms", "bundle_raster_ms", "setup_ms", "raster_ms", "depth_tiles_ms", "label_tiles_ms", "label_boxes_ms")
    rounds = {k: [] for k in names}
    for _ in range(args.rounds):
        for kind, (submit, read, fe) in kinds.items():
            dt, ts = loop(submit, args.iters, read)
            assert all(t["front_end"] == fe and t["n_frames"] == B for t in ts), kind
            rounds[kind + "_s"].append(dt)
            rounds[kind + "_host_ms"].append(med(ts, "host_ms"))
            if kind == "bundle":
                for k in ("bundle_tiles_ms", "bundle_setup_ms", "bundle_raster_ms"):
                    rounds[k].append(med(ts, k))
            elif kind == "colour":
                rounds["setup_ms"].append(med(ts, "setup_ms"))
                rounds["raster_ms"].append(med(ts, "raster_ms"))
            elif kind == "depth":
                rounds["depth_tiles_ms"].append(med(ts, "raster_ms"))
            else:
                rounds["label_tiles_ms"].append(med(ts, "tiles_ms"))
                rounds["label_boxes_ms"].append(med(ts, "boxes_ms"))
    bundle_vps = [B / t for t in rounds["bundle_s"]]
    separate_vps = [B / (c + d + l) for c, d, l in zip(rounds["colour_s"], rounds["depth_s"], rounds["label_s"])]
    replaced = [d + t + b for d, t, b in zip(rounds["depth_tiles_ms"], rounds["label_tiles_ms"], rounds["label_boxes_ms"])]
    two_tiles = [d + t for d, t in zip(rounds["depth_tiles_ms"], rounds["label_tiles_ms"])]
    m = {k: float(np.median(v)) for k, v in rounds.items()}
    out = {"metric": "bundle_views_per_s", "width": W, "height": H, "batch": args.batch, "views_per_submission": B, "iters": args.iters, "rounds": args.rounds,
           "host_threads": ctx.host_threads, "map_objects": scene.mobj_count(),
           "bundle_views_per_s": round(float(np.median(bundle_vps)), 1), "separate_views_per_s": round(float(np.median(separate_vps)), 1),
           "bundle_over_separate": round(float(np.median(bundle_vps)) / float(np.median(separate_vps)), 3),
           "bundle_faster_beyond_spread": bool(min(bundle_vps) > max(separate_vps)),
           "bundle_views_per_s_rounds": [round(v, 1) for v in bundle_vps], "separate_views_per_s_rounds": [round(v, 1) for v in separate_vps]}
    for k in names[4:]:
        out[k] = round(m[k], 4)
        out[k + "_rounds"] = [round(v, 4) for v in rounds[k]]
    out["replaced_ms_rounds"] = [round(v, 4) for v in replaced]
    out["tiles_over_replaced"] = round(m["bundle_tiles_ms"] / float(np.median(replaced)), 3)
    out["tiles_below_replaced_beyond_spread"] = bool(max(rounds["bundle_tiles_ms"]) < min(replaced))
    out["tiles_over_depth_plus_label_tiles"] = round(m["bundle_tiles_ms"] / float(np.median(two_tiles)), 3)
    out["tiles_below_depth_plus_label_tiles_beyond_spread"] = bool(max(rounds["bundle_tiles_ms"]) < min(two_tiles))
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
