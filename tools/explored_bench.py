#!/usr/bin/env python3
"""explored_bench.py — the explored-map kernels next to their yardsticks on one MI355X, in one run.

    python tools/explored_bench.py [--width 1280 --height 800] [--batch 1000] [--iters 10] [--rounds 3]

Workload: the 1 000 views of tests/golden/campath_seed1993.f32 over the synthetic e1m1-like map (seed 1993), one session of --batch frames.
Prints one JSON line.
 (a) the seen set.  One label submission of the batch, then per round --iters calls of dg_slot_seen_lines(run_len = batch):
       seen_lines_ms, seen_accumulate_ms   medians of dg_ctx_seen_kernel_ms (events on the dispatches); *_rounds: the per-round medians
       seen_read_tb_per_s                  3 * W * H * batch bytes (the id and cls planes) over seen_lines_ms
       stream_read_ms, stream_read_tb_per_s   tools/microbench/stream_read over the same byte count, run as a child between the rounds
       label_boxes_ms                      dg_label_boxes of the same submission (dg_slot_label_timing): it reads the same bytes
       seen_call_ms                        wall time of one dg_slot_seen_lines call (kernels + the copies of the small rows)
 (b) the map frames.  Per round --iters replays of one explored submission (masks: the session's accumulated rows) and of one
     dg_submit_map_views submission of the same views:
       explored_kernel_ms, map_kernel_ms   medians of dg_slot_timing raster_ms (dg_map_explored + arrow / dg_map_copy + dg_map_arrow)
       explored_frames_per_s, map_frames_per_s   frames / wall time of submit + wait, two slots round robin
       cover_upload_ms                     setup_ms of the submission that built the cover; lines_seen: popcount of the last mask row
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_READ = os.path.join(ROOT, "tools", "microbench", "stream_read")


def stream_read(n_bytes: int) -> dict:
    """tools/microbench/stream_read as a child process (built with hipcc when it is not there)."""
    if not os.path.exists(STREAM_READ):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", STREAM_READ, STREAM_READ + ".hip"])
    r = subprocess.run([STREAM_READ, str(n_bytes), "10"], capture_output=True, text=True, timeout=300, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


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
    W, H, F = args.width, args.height, args.batch
    views = dg.make_views(np.resize(path, (F, 8)))
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=2, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)
    plane_bytes = 3 * W * H * F
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "explored_map", "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds, "seen_words": dg.seen_words(scene),
           "plane_bytes": plane_bytes}

    # (a) the seen set of one label session
    ctx.submit_labels(0, views)
    ctx.wait(0)
    boxes_ms = ctx.label_timing(0)["boxes_ms"]
    acc = ctx.slot_seen_lines(0, 0, F, F)                      # warm-up: the seg table, the scratch rows, code resident
    rounds = {"seen_lines_ms": [], "seen_accumulate_ms": [], "seen_call_ms": [], "stream_read_ms": [], "explored_kernel_ms": [], "map_kernel_ms": [],
              "explored_fps": [], "map_fps": []}
    for _ in range(args.rounds):
        ls, as_, cs = [], [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            ctx.slot_seen_lines(0, 0, F, F)
            cs.append((time.perf_counter() - t0) * 1e3)
            t = ctx.seen_kernel_ms()
            ls.append(t["lines_ms"])
            as_.append(t["accumulate_ms"])
        rounds["seen_lines_ms"].append(med(ls))
        rounds["seen_accumulate_ms"].append(med(as_))
        rounds["seen_call_ms"].append(med(cs))
        rounds["stream_read_ms"].append(stream_read(plane_bytes)["ms_median"])
    masks = acc["upto"]
    out["lines_seen"] = int(acc["total"][-1])

    # (b) explored frames next to the map view's frames (slot 0's label planes are replaced from here on)
    ctx.submit_explored_map(0, views, masks)
    ctx.wait(0)
    out["cover_upload_ms"] = round(ctx.timing(0)["setup_ms"], 4)
    ctx.submit_map(1, views)
    ctx.wait(1)
    out["layer_build_ms"] = round(ctx.timing(1)["setup_ms"], 4)

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

    for _ in range(args.rounds):
        rounds["explored_fps"].append(frames_per_s(lambda s: ctx.submit_explored_map(s, views, masks)))
        rounds["map_fps"].append(frames_per_s(lambda s: ctx.submit_map(s, views)))
        ctx.submit_explored_map(0, views, masks)
        ctx.submit_map(1, views)
        rounds["explored_kernel_ms"].append(replay_ms(0))
        rounds["map_kernel_ms"].append(replay_ms(1))
    m = {k: med(v) for k, v in rounds.items()}
    for k in ("seen_lines_ms", "seen_accumulate_ms", "seen_call_ms", "stream_read_ms", "explored_kernel_ms", "map_kernel_ms"):
        out[k] = round(m[k], 4)
        out[k + "_rounds"] = [round(v, 4) for v in rounds[k]]
    out["label_boxes_ms"] = round(boxes_ms, 4)
    out["seen_read_tb_per_s"] = round(plane_bytes / (m["seen_lines_ms"] * 1e-3) / 1e12, 3)
    out["stream_read_tb_per_s"] = round(plane_bytes / (m["stream_read_ms"] * 1e-3) / 1e12, 3)
    out["seen_lines_over_stream_read"] = round(m["seen_lines_ms"] / m["stream_read_ms"], 3)
    out["seen_lines_over_label_boxes"] = round(m["seen_lines_ms"] / boxes_ms, 3)
    out["explored_over_map_kernel"] = round(m["explored_kernel_ms"] / m["map_kernel_ms"], 3)
    out["explored_write_tb_per_s"] = round(plane_bytes / (m["explored_kernel_ms"] * 1e-3) / 1e12, 3)
    out["map_write_tb_per_s"] = round(plane_bytes / (m["map_kernel_ms"] * 1e-3) / 1e12, 3)
    out["explored_frames_per_s"] = round(m["explored_fps"], 1)
    out["map_frames_per_s"] = round(m["map_fps"], 1)
    out["explored_frames_per_s_rounds"] = [round(v, 1) for v in rounds["explored_fps"]]
    out["map_frames_per_s_rounds"] = [round(v, 1) for v in rounds["map_fps"]]
    print(json.dumps(out))
    ctx.close()
    scene.close()


if __name__ == "__main__":
    main()
