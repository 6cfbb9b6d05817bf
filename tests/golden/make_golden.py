#!/usr/bin/env python3
"""Regenerates the committed fixtures under tests/golden/ (run from the repo root, CPU only).

What is pinned and by what:
  * synth_wad.json       sha256 of the synthetic IWADs (pins the generator, not the renderer): seed 1993 (bench map), seed 1994
                         (heavy map), seed 1995 (the "vanilla-shaped" variant: arbitrary integer vertices and wall angles, rounded
                         BSP splits, closed doors, 1-degree thing angles, patches with negative / past-the-bottom origins)
  * campath_*.f32        the 1000-frame camera paths: raw little-endian f32 [1000][8] =
                         x, y, angle, cos, sin, cos(-a), sin(-a), floor_height (camera_path.view_record)
  * frames_*.json        sha256 of ORACLE frames (oracle/doomref.c) at sampled path frames and sizes
  * checksums_*.json     dg_frame_checksums value (include/doomgpu.h) of EVERY oracle frame of the 1000-frame paths at
                         1280x800 (the bench size): the GPU tier compares all of them without moving a frame over PCIe
  * checksums_map*.u64   the same, as raw little-endian u64, for every frame bench.py renders: one file per distinct (map, camera
                         path, frame size) that bench.rank_plan gives the 8 ranks of configs 1-5 (tests/rank_plans.py)
  * rank_plans.json      what each of those files pins: map, camera, path seed, size, and the sha256 of the path, built as bench
                         builds it (here with the oracle's floor_height_at)

The reference itself ships no fixtures and cannot be run here, so these vectors pin the in-repo CPU
restatement against regressions ("parity unpinned" w.r.t. the Rust binary).
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import doomref  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import rank_plans  # noqa: E402

sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
cp = importlib.import_module("doom-rust-renderer_amd.camera_path")
OUT = os.path.dirname(os.path.abspath(__file__))

SIZES = {"320x200": list(range(0, 1000, 25)), "1280x800": [0, 100, 297, 323, 623, 728], "1024x768": [5, 505], "2560x1600": [728]}


def full_path_checksums(wad, path, W, H):
    """Checksum (doom-rust-renderer_amd.frame_checksum = dg_frame_checksums' formula) of every oracle frame of the path, as hex
    strings; the frames are sharded over threads, one oracle scene each (its lazy caches are per scene)."""
    import threading
    dgpy = importlib.import_module("doom-rust-renderer_amd")
    n = min(8, os.cpu_count() or 1)
    scenes = [doomref.Scene(wad, "e1m1") for _ in range(n)]
    out = [None] * len(path)

    def work(t):
        buf = np.empty(3 * W * H, dtype=np.uint8)
        for i in range(t, len(path), n):
            scenes[t].render(W, H, path[i], out=buf.ctypes.data)
            out[i] = f"{dgpy.frame_checksum(buf):016x}"
    th = [threading.Thread(target=work, args=(t,)) for t in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for sc in scenes:
        sc.close()
    return out


def write_rank_plan_fixtures():
    """One checksum vector per plan of tests/rank_plans.py that no older fixture pins already, and the index that describes them."""
    scenes, index = {}, {}
    for plan in sorted(rank_plans.plans(), key=str):
        if plan in rank_plans.LEGACY:
            continue
        map_seed, heavy, camera, path_seed, size = plan
        if (map_seed, heavy) not in scenes:
            wad = sw.build_synth_iwad(map_seed, heavy=heavy)
            scenes[(map_seed, heavy)] = (wad, doomref.Scene(wad, "e1m1"))
        wad, sc = scenes[(map_seed, heavy)]
        path = rank_plans.bench_path(plan, sc, cp, sw)
        W, H = map(int, size.split("x"))
        sums = full_path_checksums(wad, path[:1] if camera == "start" else path, W, H)
        name = rank_plans.fixture_name(plan)
        np.array([int(h, 16) for h in sums], dtype="<u8").tofile(os.path.join(OUT, name))
        index[name] = {"map_seed": map_seed, "heavy": heavy, "camera": camera, "path_seed": path_seed, "size": size,
                       "path_sha256": rank_plans.path_sha256(path)}
        print("wrote", name, flush=True)
    json.dump(index, open(os.path.join(OUT, rank_plans.INDEX), "w"), indent=1, sort_keys=True)
    for _, sc in scenes.values():
        sc.close()


def main():
    wads = {}
    for seed, heavy, vanilla in ((1993, False, False), (1994, True, False), (1995, False, True)):
        wad = sw.build_synth_iwad(seed, heavy=heavy, vanilla=vanilla)
        wads[str(seed)] = {"sha256": hashlib.sha256(wad).hexdigest(), "bytes": len(wad), "heavy": heavy}
        if vanilla:
            wads[str(seed)]["vanilla"] = True
        sc = doomref.Scene(wad, "e1m1")
        path = cp.make_camera_path(sw.synth_route(seed, heavy=heavy, vanilla=vanilla), lambda x, y, d: sc.floor_height_at(x, y, d), 1000)
        path.astype("<f4").tofile(os.path.join(OUT, f"campath_seed{seed}.f32"))
        frames = {}
        sizes = SIZES if not heavy else {"320x200": list(range(0, 1000, 100)), "1280x800": [250]}
        for size, idx in sizes.items():
            W, H = map(int, size.split("x"))
            frames[size] = {str(i): hashlib.sha256(sc.render(W, H, path[i])).hexdigest() for i in idx}
        # animated flats: timestamp-dependent frame (flats.rs:103-111)
        W, H = 320, 200
        frames["320x200@t=0.4"] = {str(i): hashlib.sha256(sc.render(W, H, list(path[i]) + [0.4])).hexdigest() for i in (50, 240, 500)}
        json.dump(frames, open(os.path.join(OUT, f"frames_seed{seed}.json"), "w"), indent=1, sort_keys=True)
        sc.close()
        json.dump({"size": "1280x800", "checksums": full_path_checksums(wad, path, 1280, 800)},
                  open(os.path.join(OUT, f"checksums_seed{seed}_1280x800.json"), "w"))
    json.dump(wads, open(os.path.join(OUT, "synth_wad.json"), "w"), indent=1, sort_keys=True)
    write_rank_plan_fixtures()


if __name__ == "__main__":
    main()
