"""The frames bench.py renders, one plan per distinct (map, camera, frame size): bench.rank_plan over 8 ranks x configs 1-5, and the
oracle checksums that pin each plan's 1 000 frames (tests/golden/, written by tests/golden/make_golden.py).

A plan's fixture is a vector of raw little-endian u64, dg_frame_checksums' value of every oracle frame in path order
(checksums_map*.u64; the start view, the same frame 1 000 times, keeps one), and its entry in rank_plans.json: map_seed, heavy, camera
("path" | "start"), path_seed (None for the start view), size and path_sha256 (sha256 of the little-endian f32 bytes of the 1000 x 8 path
bench builds)."""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

WORLD = 8
BENCH_CONFIGS = (1, 2, 3, 4, 5)
# The one plan an older fixture already pins (the light map's own route at the bench size): its checksums and its path file are reused
LEGACY = {(1993, False, "path", 1993, "1280x800"): ("checksums_seed1993_1280x800.json", "campath_seed1993.f32")}
INDEX = "rank_plans.json"


def plans():
    """{plan: [(config, rank), ...]} with plan = (map_seed, heavy, camera, path_seed or None, "WxH"), for every rank of an 8-GPU run."""
    out = {}
    for config in BENCH_CONFIGS:
        _, W, H, _, _, camera = bench.CONFIGS[config]
        for rank in range(WORLD):
            (map_seed, heavy), path_seed = bench.rank_plan(rank, WORLD, config)
            key = (map_seed, heavy, camera, path_seed if camera == "path" else None, f"{W}x{H}")
            out.setdefault(key, []).append((config, rank))
    return out


def plans_of_config(config: int):
    return sorted((k for k, users in plans().items() if any(c == config for c, _ in users)), key=str)


def fixture_name(plan) -> str:
    if plan in LEGACY:
        return LEGACY[plan][0]
    map_seed, _, camera, path_seed, size = plan
    return f"checksums_map{map_seed}_{'start' if camera == 'start' else f'path{path_seed}'}_{size}.u64"


def bench_path(plan, scene, camera_path, synth):
    """The 1000 x 8 f32 path bench.DoomGpuBackend.load builds for the plan, with `scene`'s floor_height_at (the product's or the oracle's)."""
    import numpy as np
    map_seed, heavy, camera, path_seed, _ = plan
    if camera == "start":
        x, y, ang = scene.player_start()
        return np.tile(camera_path.view_record(x, y, ang, scene.floor_height_at(x, y, 0.0)), (bench.PATH_FRAMES, 1))
    return camera_path.make_camera_path(bench.seeded_route(_route(synth, map_seed, heavy), path_seed), lambda x, y, d: scene.floor_height_at(x, y, d), bench.PATH_FRAMES)


@functools.lru_cache(maxsize=None)
def _route(synth, map_seed, heavy):
    return synth.synth_route(map_seed, heavy=heavy)


def path_sha256(path) -> str:
    return hashlib.sha256(path.astype("<f4").tobytes()).hexdigest()


def load_fixture(plan) -> dict:
    """The plan's index entry + its checksums as hex strings (the legacy file holds only size + checksums; its path is campath_seed1993.f32)."""
    import numpy as np
    name = fixture_name(plan)
    if plan not in LEGACY:
        g = dict(json.load(open(os.path.join(GOLDEN, INDEX)))[name])
        g["checksums"] = [f"{int(v):016x}" for v in np.fromfile(os.path.join(GOLDEN, name), dtype="<u8")]
        return g
    map_seed, heavy, camera, path_seed, size = plan
    raw = open(os.path.join(GOLDEN, LEGACY[plan][1]), "rb").read()
    return dict(json.load(open(os.path.join(GOLDEN, name))), map_seed=map_seed, heavy=heavy, camera=camera, path_seed=path_seed,
                path_sha256=hashlib.sha256(raw).hexdigest())


def frame_checksums(fixture) -> list:
    """The 1 000 expected checksums, hex (the start view's one repeated)."""
    c = fixture["checksums"]
    return c * bench.PATH_FRAMES if fixture["camera"] == "start" else c
