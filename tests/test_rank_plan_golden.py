"""The oracle checksum fixtures of every frame bench.py renders (tests/rank_plans.py: one per distinct (map, camera, frame size) of the 8
ranks of configs 1-5) stay honest on the CPU: each pins the path bench builds and the oracle's frames on it; the GPU tier
(test_rank_plans_gpu.py) then compares all 1 000 frames of every plan with them."""
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import rank_plans

PLANS = sorted(rank_plans.plans(), key=str)


def _id(plan):
    return os.path.splitext(rank_plans.fixture_name(plan))[0]


def test_the_fixtures_are_exactly_the_plans_bench_renders():
    """A new config, rank count or path seed in bench.py fails here until its frames are pinned (make_golden.py writes them)."""
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(rank_plans.GOLDEN, "checksums_map*"))}
    wanted = {rank_plans.fixture_name(p) for p in PLANS if p not in rank_plans.LEGACY}
    assert on_disk == wanted
    assert set(json.load(open(os.path.join(rank_plans.GOLDEN, rank_plans.INDEX)))) == wanted
    assert len(PLANS) == 29 and len(wanted) == 28


N_ORACLES = max(1, min(4, os.cpu_count() or 1))       # oracle scenes per map: the sampled frames are rendered on that many threads


@pytest.fixture(scope="module")
def scenes(dg, oracle, synth):
    """(map_seed, heavy) -> (product scene, [oracle scene per thread]) (an oracle scene's lazy caches are its own: one per thread)"""
    out = {}
    for (map_seed, heavy) in {(p[0], p[1]) for p in PLANS}:
        wad = synth.build_synth_iwad(map_seed, heavy=heavy)
        out[(map_seed, heavy)] = (dg.Scene(wad, "e1m1"), [oracle.Scene(wad, "e1m1") for _ in range(N_ORACLES)])
    yield out
    for sc, oscs in out.values():
        sc.close()
        for osc in oscs:
            osc.close()


@pytest.mark.parametrize("plan", PLANS, ids=_id)
def test_the_fixture_pins_the_path_bench_builds_and_the_oracle_s_frames(dg, synth, campath_mod, scenes, plan):
    map_seed, heavy, camera, path_seed, size = plan
    g = rank_plans.load_fixture(plan)
    assert (g["map_seed"], g["heavy"], g["camera"], g["path_seed"], g["size"]) == plan
    assert len(g["checksums"]) == (1 if camera == "start" else 1000)
    sc, oscs = scenes[(map_seed, heavy)]
    path = rank_plans.bench_path(plan, oscs[0], campath_mod, synth)
    assert rank_plans.path_sha256(path) == g["path_sha256"], "the oracle's floor heights give another path"
    assert rank_plans.path_sha256(rank_plans.bench_path(plan, sc, campath_mod, synth)) == g["path_sha256"], "the product's floor heights give another path"
    W, H = map(int, size.split("x"))
    sums = rank_plans.frame_checksums(g)
    idx = [0] if camera == "start" else list(range(3, 1000, 111))
    with ThreadPoolExecutor(N_ORACLES) as pool:
        got = list(pool.map(lambda t: [(i, f"{dg.frame_checksum(oscs[t].render(W, H, path[i])):016x}") for i in idx[t::N_ORACLES]], range(N_ORACLES)))
    for i, c in sorted(x for part in got for x in part):
        assert c == sums[i], f"frame {i}"
    assert sum(len(part) for part in got) == len(idx)
