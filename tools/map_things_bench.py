#!/usr/bin/env python3
"""map_things_bench.py — the map frames' kernels with the things phase next to the plain kernels on one MI355X, in one run.

    python tools/map_things_bench.py [--width 1280 --height 800] [--batch 1000] [--scale 0.25] [--iters 5] [--rounds 3]
                                     [--synth-map 2002:32x24:500] [--only small|large] [--parent-lib PATH/libdoomgpu.so]

Workload: --batch frames per submission (a full max_batch), heading up with the arrow, no mask; on the small map (build_synth_iwad(1993),
40 map objects, the views of tests/golden/campath_seed1993.f32) and on the generated map of --synth-map (SEED:COLUMNSxROWS:THINGS, heavy +
vanilla: doom2's scale, 500 map objects; views on its vertices).  Prints one JSON line per map.  Per kind and round --iters replays of
one submission (medians of dg_slot_timing raster_ms, events on the dispatches):
    ego_plain, floor_plain              dg_ego_tiles / dg_floor_map_tiles: the plain submissions of this library
    ego_none, floor_none                dg_ego_thing_tiles / dg_floor_thing_tiles with a marker table whose flags are all 0: every item is
                                        looked at, no object is shown
    ego_all, floor_all                  ... with every object marked with box and heading, each frame with a pose entry for every third object
    parent_ego_plain, parent_floor_plain   the plain submissions through --parent-lib (the parent commit's library, built apart), measured
                                        by a child process of this tool in the same run; absent without the option
"""
import argparse
import ctypes
import importlib
import json
import os
import struct
import subprocess
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


def measure(dg, name, wad, views, args, plain_only):
    W, H, F = args.width, args.height, args.batch
    scene = dg.Scene(wad, "e1m1")
    n_obj = scene.mobj_count()
    ctx = dg.Context(W, H, max_batch=F, slots=1, front_end=dg.DG_FE_HOST)
    params = dg.DgEgoMap(args.scale, dg.DG_EGO_ROTATE | dg.DG_EGO_ARROW)
    med = lambda v: float(np.median(v))                       # noqa: E731
    out = {"metric": "map_things", "map": name, "width": W, "height": H, "batch": F, "scale": args.scale, "iters": args.iters, "rounds": args.rounds,
           "map_objects": n_obj, "lib": dg.LIB_PATH}

    def replay_ms():
        ks = []
        for _ in range(args.iters):
            ctx.replay(0)
            ctx.wait(0)
            ks.append(ctx.timing(0)["raster_ms"])
        return med(ks)

    placed = scene.mobj_poses()
    poses = None if plain_only else [[(i, float(placed["x"][i]) + 8.0 + (f % 16), float(placed["y"][i]) - 4.0, 0.05 * f) for i in range(f % 3, n_obj, 3)] for f in range(F)]
    tables = {"plain": None} if plain_only else {"plain": None, "none": [(16, 0x00ff00, 0)] * n_obj, "all": [(16 + 8 * (i % 3), 0x40ff40 + i, 3) for i in range(n_obj)]}
    rounds = {}
    for _ in range(args.rounds):
        for kind, table in tables.items():
            if not plain_only:
                scene.set_map_markers(table)
            ctx.upload_scene(scene)                           # (a ctx takes the marker table here)
            for base in ("ego", "floor"):
                if kind == "plain":
                    (ctx.submit_ego_map if base == "ego" else ctx.submit_floor_map)(0, views, params)
                elif base == "ego":
                    ctx.submit_ego_map_things(0, views, params, None, None, poses if kind == "all" else None)
                else:
                    ctx.submit_floor_map_things(0, views, params, None, None, None, poses if kind == "all" else None)
                ctx.wait(0)
                rounds.setdefault(f"{base}_{kind}", []).append(replay_ms())
    out["kernel_ms"] = {k: round(med(v), 4) for k, v in rounds.items()}
    out["kernel_ms_rounds"] = {k: [round(t, 4) for t in v] for k, v in rounds.items()}
    ctx.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--synth-map", default="2002:32x24:500")
    ap.add_argument("--only", choices=["small", "large"], default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--plain-only", action="store_true", help="the plain submissions alone (what a child started for --parent-lib runs)")
    args = ap.parse_args()
    dg = importlib.import_module("doom-rust-renderer_amd")
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    if args.plain_only:                                       # a library from before the markers: bind what it has
        have = ctypes.CDLL(dg.LIB_PATH)
        for n in [n for n in dg._SIGNATURES if not hasattr(have, n)]:
            del dg._SIGNATURES[n]
    maps = []
    if args.only != "large":
        path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
        maps.append(("small (seed 1993)", sw.build_synth_iwad(1993), lambda wad: dg.make_views(np.resize(path, (args.batch, 8)))))
    if args.only != "small":
        seed, grid, things = args.synth_map.split(":")
        maps.append((f"synth {args.synth_map}", sw.build_synth_iwad(int(seed), heavy=True, vanilla=True, grid=tuple(int(v) for v in grid.split("x")), n_things=int(things)),
                     lambda wad: vertex_views(dg, sw, wad, args.batch)))
    results = [measure(dg, name, wad, views(wad), args, args.plain_only) for name, wad, views in maps]
    if args.parent_lib and not args.plain_only:               # a fresh process: a library is loaded once per process
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only"] + [a for a in sys.argv[1:] if a != "--plain-only"]
        i = cmd.index("--parent-lib")
        del cmd[i:i + 2]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, DOOMGPU_LIB=os.path.abspath(args.parent_lib)), timeout=900)
        if r.returncode != 0:
            raise SystemExit("the child for --parent-lib failed:\n" + r.stderr[-2000:])
        for res, line in zip(results, [l for l in r.stdout.splitlines() if l.startswith("{")]):
            child = json.loads(line)
            res["kernel_ms"].update({"parent_" + k: v for k, v in child["kernel_ms"].items()})
            res["kernel_ms_rounds"].update({"parent_" + k: v for k, v in child["kernel_ms_rounds"].items()})
            res["parent_lib"] = child["lib"]
    for res in results:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
