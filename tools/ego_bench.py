#!/usr/bin/env python3
"""ego_bench.py — the player-centred map frames' kernel next to its yardsticks on one MI355X, in one run.

    python tools/ego_bench.py [--width 1280 --height 800] [--scale 0.25] [--batch 1000] [--iters 10] [--rounds 3]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), --batch frames per
submission, heading up with the arrow, every line (no mask) and, as a second figure, the mask rows of a label session of the same views.
Prints one JSON line.  Per round --iters replays of one submission each (medians of dg_slot_timing raster_ms, events on the dispatches):
    ego_kernel_ms, ego_masked_kernel_ms   dg_ego_tiles
    map_kernel_ms                         dg_map_copy + dg_map_arrow for the same frame count: the pure write floor
    explored_kernel_ms                    dg_map_explored + arrow (the session's rows)
and frames / wall time of submit + wait, two slots round robin: ego_frames_per_s, map_frames_per_s, explored_frames_per_s.
table_upload_ms: setup_ms of the submission that uploaded the line table.  The map and explored calls need frames of at least 40 x 40.
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
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    W, H, F = args.width, args.height, args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)
    params = dg.DgEgoMap(args.scale, dg.DG_EGO_ROTATE | dg.DG_EGO_ARROW)
    frame_bytes = 3 * W * H * F
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "ego_map", "width": W, "height": H, "scale": args.scale, "batch": F, "iters": args.iters, "rounds": args.rounds,
           "seen_words": dg.seen_words(scene), "frame_bytes": frame_bytes}

    # the session's mask rows: one label submission of the batch
    ctx.submit_labels(0, views)
    masks = ctx.slot_seen_lines(0, 0, F, F)["upto"]
    out["lines_seen"] = int(np.unpackbits(masks[-1].view(np.uint8)).sum())

    ctx.submit_ego_map(0, views, params)
    ctx.wait(0)
    out["table_upload_ms"] = round(ctx.timing(0)["setup_ms"], 4)
    ctx.submit_map(1, views)
    ctx.wait(1)
    ctx.submit_explored_map(1, views, masks)
    ctx.wait(1)

    def frames_per_s(submit):
        for i in range(2):
            submit(i % 2)
        ctx.wait(0)
        ctx.wait(1)
        t0 = time.perf_counter()
        for i in range(args.iters):
            submit(i % 2)
        ctx.wait(0)
        ctx.wait(1)
        return args.iters * F / (time.perf_counter() - t0)

    def replay_ms(slot):
        ks = []
        for _ in range(args.iters):
            ctx.replay(slot)
            ctx.wait(slot)
            ks.append(ctx.timing(slot)["raster_ms"])
        return med(ks)

    kinds = {"ego": lambda s: ctx.submit_ego_map(s, views, params), "ego_masked": lambda s: ctx.submit_ego_map(s, views, params, masks),
             "map": lambda s: ctx.submit_map(s, views), "explored": lambda s: ctx.submit_explored_map(s, views, masks)}
    rounds = {k + "_kernel_ms": [] for k in kinds}
    rounds.update({k + "_fps": [] for k in kinds})
    for _ in range(args.rounds):
        for k, submit in kinds.items():
            rounds[k + "_fps"].append(frames_per_s(submit))
            submit(0)
            rounds[k + "_kernel_ms"].append(replay_ms(0))
    m = {k: med(v) for k, v in rounds.items()}
    for k in kinds:
        out[k + "_kernel_ms"] = round(m[k + "_kernel_ms"], 4)
        out[k + "_kernel_ms_rounds"] = [round(v, 4) for v in rounds[k + "_kernel_ms"]]
        out[k + "_frames_per_s"] = round(m[k + "_fps"], 1)
        out[k + "_frames_per_s_rounds"] = [round(v, 1) for v in rounds[k + "_fps"]]
    out["ego_over_map_kernel"] = round(m["ego_kernel_ms"] / m["map_kernel_ms"], 3)
    out["ego_over_explored_kernel"] = round(m["ego_kernel_ms"] / m["explored_kernel_ms"], 3)
    out["ego_write_tb_per_s"] = round(frame_bytes / (m["ego_kernel_ms"] * 1e-3) / 1e12, 3)
    out["map_write_tb_per_s"] = round(frame_bytes / (m["map_kernel_ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
