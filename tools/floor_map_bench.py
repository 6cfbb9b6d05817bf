#!/usr/bin/env python3
"""floor_map_bench.py — the floor-textured map frames' kernel next to its yardsticks on one MI355X, in one run.

    python tools/floor_map_bench.py [--width 1280 --height 800] [--scales 0.1,1,8] [--batch 512] [--iters 10] [--rounds 3]
                                    [--synth-map 2002:32x24:500] [--only light|synth]

Workload: --batch frames per submission (a full max_batch), heading up with the arrow, no mask and, as a second figure, random mask
rows; on the light map (build_synth_iwad(1993), the views of tests/golden/campath_seed1993.f32) and on the generated map of --synth-map
(SEED:COLUMNSxROWS:THINGS, heavy + vanilla; views on its vertices — tree depth is the descent's cost).  Prints one JSON line per map.
Per scale and round --iters replays of one submission each (medians of dg_slot_timing raster_ms, events on the dispatches):
    floor_kernel_ms, floor_masked_kernel_ms    dg_floor_map_tiles
    ego_kernel_ms                              dg_ego_tiles on the same views and parameters: the same lines, no floor
    colour_raster_ms                           raster_ms of a colour submission (dg_submit_views) of the same views, light map only
floor_gb_per_s: bytes of frame stored per second by dg_floor_map_tiles.  table_upload_ms: setup_ms of the submission that uploaded the
tables.
"""
import argparse
import importlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vertex_views(dg, sw, wad, n):
    """n views on the map's vertices, spread over the lump, headings turning."""
    d = sw.wad_directory(wad)
    i = next(k for k, (name, _, _) in enumerate(d) if name == "E1M1")
    _, off, size = d[i + 4]
    verts = list(struct.iter_unpack("<hh", wad[off:off + size - size % 4]))
    arr = (dg.DgView * n)()
    for k in range(n):
        x, y = verts[(k * 7919) % len(verts)]
        arr[k] = dg.DgView(float(x) + 3.5, float(y) - 2.25, 0.1 * k, 0, 0, 0, 0, 0, 0.1 * k, 0)
    return arr


def measure(dg, name, wad, views, args, colour):
    W, H, F = args.width, args.height, args.batch
    scene = dg.Scene(wad, "e1m1")
    ctx = dg.Context(W, H, max_batch=F, slots=1, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)
    words = dg.seen_words(scene)
    masks = np.random.default_rng(7).integers(0, 1 << 32, (F, words), dtype=np.uint64).astype(np.uint32)
    frame_bytes = 3 * W * H * F
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "floor_map", "map": name, "width": W, "height": H, "batch": F, "iters": args.iters, "rounds": args.rounds,
           "sectors": scene.sector_count(), "seen_words": words, "frame_bytes": frame_bytes, "scales": {}}

    def replay_ms():
        ks = []
        for _ in range(args.iters):
            ctx.replay(0)
            ctx.wait(0)
            ks.append(ctx.timing(0)["raster_ms"])
        return med(ks)

    for scale in args.scales:
        params = dg.DgEgoMap(scale, dg.DG_EGO_ROTATE | dg.DG_EGO_ARROW)
        kinds = {"floor": lambda: ctx.submit_floor_map(0, views, params), "floor_masked": lambda: ctx.submit_floor_map(0, views, params, masks),
                 "ego": lambda: ctx.submit_ego_map(0, views, params)}
        if colour:
            kinds["colour"] = lambda: ctx.submit(0, views)
        rounds = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k, submit in kinds.items():
                submit()
                ctx.wait(0)
                if "table_upload_ms" not in out and k == "floor":
                    out["table_upload_ms"] = round(ctx.timing(0)["setup_ms"], 4)
                rounds[k].append(replay_ms())
        m = {k: med(v) for k, v in rounds.items()}
        s = {("colour_raster_ms" if k == "colour" else k + "_kernel_ms"): round(v, 4) for k, v in m.items()}
        s.update({k + "_rounds": [round(v, 4) for v in r] for k, r in rounds.items()})
        s["floor_over_ego_kernel"] = round(m["floor"] / m["ego"], 2)
        s["floor_gb_per_s"] = round(frame_bytes / (m["floor"] * 1e-3) / 1e9, 1)
        s["floor_us_per_frame"] = round(1e3 * m["floor"] / F, 3)
        out["scales"][str(scale)] = s
    ctx.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--scales", type=lambda s: [float(v) for v in s.split(",")], default=[0.1, 1.0, 8.0])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--synth-map", default="2002:32x24:500")
    ap.add_argument("--only", choices=["light", "synth"], default=None)
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    if args.only != "synth":
        path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
        print(json.dumps(measure(dg, "light (seed 1993)", sw.build_synth_iwad(1993), dg.make_views(np.resize(path, (args.batch, 8))), args, True)), flush=True)
    if args.only != "light":
        seed, grid, things = args.synth_map.split(":")
        wad = sw.build_synth_iwad(int(seed), heavy=True, vanilla=True, grid=tuple(int(v) for v in grid.split("x")), n_things=int(things))
        print(json.dumps(measure(dg, f"synth {args.synth_map}", wad, vertex_views(dg, sw, wad, args.batch), args, False)), flush=True)


if __name__ == "__main__":
    main()
