"""Every frame bench.py renders, as bench renders it: for each rank plan of configs 1-5 (tests/rank_plans.py) the backend is loaded the way
bench.py loads it (same scene, path, batch, slots), its path is checked against the fixture's hash, and all 1 000 frames go through each
forced front end and through DG_FE_AUTO submitted as bench's timed loop submits them; the device checksums of every frame are compared
with the oracle's (tests/golden/checksums_*: rank_plans.load_fixture), so no frame crosses PCIe."""
import time

import pytest

import rank_plans
from rank_plans import bench

pytestmark = pytest.mark.gpu

FORCED = ("host", "device", "segs")
# the workgroup-to-frame mapping of dg_raster_tiles not taken by default at the config's size (kernels.hip: launch_raster), on its first plan
OTHER_XCD_MAPPING = {3: "0", 5: "1"}


class _MemoSynth:
    """The backend's synthetic-map generator with its two pure functions memoised: every backend of a plan loads the same WAD and route,
    and building them takes longer than rendering a plan's frames."""

    def __init__(self, sw):
        self._sw, self._memo = sw, {}

    def _get(self, name, *a, **kw):
        key = (name, a, tuple(sorted(kw.items())))
        if key not in self._memo:
            self._memo[key] = getattr(self._sw, name)(*a, **kw)
        return self._memo[key]

    def build_synth_iwad(self, *a, **kw):
        return self._get("build_synth_iwad", *a, **kw)

    def synth_route(self, *a, **kw):
        return self._get("synth_route", *a, **kw)


@pytest.fixture(scope="module")
def memo_synth(synth):
    return _MemoSynth(synth)


def _load(config, plan, front_end, memo_synth):
    map_seed, heavy, camera, path_seed, _ = plan
    be = bench.DoomGpuBackend(bench.parse_args(["--config", str(config), "--front-end", front_end]), 0)
    be.sw = memo_synth
    ctx = be.load((map_seed, heavy), path_seed if path_seed is not None else 1993, camera)
    return be, ctx


def _check_slot(be, ctx, s, want, label):
    B = be.args.batch
    got = [f"{int(v):016x}" for v in ctx.frame_checksums(s, 0, B)]
    frames = [(be.batch_first[s] + k) % bench.PATH_FRAMES for k in range(B)]
    bad = [i for k, i in enumerate(frames) if got[k] != want[i]]
    assert not bad, f"{label}: frames {bad[:10]} differ from the oracle"
    return set(frames)


def _forced(dg, be, ctx, fe, want, label):
    """Every slot submitted back to back, then waited for and compared: the whole path at least once."""
    code = {"host": dg.DG_FE_HOST, "device": dg.DG_FE_DEVICE, "segs": dg.DG_FE_DEVICE_SEGS}[fe]
    for s in range(be.n_slots):
        ctx.submit(s, be.views[s])
    seen = set()
    for s in range(be.n_slots):
        ctx.wait(s)
        assert ctx.timing(s)["front_end"] == code, f"{label}: slot {s} ran front end {ctx.timing(s)['front_end']}"
        seen |= _check_slot(be, ctx, s, want, label)
    assert len(seen) == bench.PATH_FRAMES


def _pipelined(be, ctx, want, label, steps=2):
    """bench.py's timed loop (one_pass): batch g goes to slot g % slots, which is waited for (and compared) just before it is submitted
    again, so the next batches are in flight while one is looked at."""
    n = be.n_slots
    batches = steps * (bench.PATH_FRAMES // be.args.batch)
    ran, used, seen = [False] * n, [], set()
    for g in range(max(batches, n)):
        s = g % n
        if ran[s]:
            ctx.wait(s)
            used.append(ctx.timing(s)["front_end"])
            seen |= _check_slot(be, ctx, s, want, f"{label}, batch {g - n}")
        ctx.submit(s, be.views[s])
        ran[s] = True
    for s in range(n):
        ctx.wait(s)
        used.append(ctx.timing(s)["front_end"])
        seen |= _check_slot(be, ctx, s, want, label)
    assert len(seen) == bench.PATH_FRAMES
    return used


@pytest.mark.parametrize("config", rank_plans.BENCH_CONFIGS, ids=lambda c: f"rank_plans_config{c}")
def test_every_frame_of_every_rank_plan_through_every_front_end(dg, memo_synth, monkeypatch, config):
    t0 = time.time()
    plans = rank_plans.plans_of_config(config)
    assert plans
    for n, plan in enumerate(plans):
        g = rank_plans.load_fixture(plan)
        want = rank_plans.frame_checksums(g)
        name = rank_plans.fixture_name(plan)
        for fe in FORCED + ("auto",):
            label = f"config {config}, {name}, front end {fe}"
            be, ctx = _load(config, plan, fe, memo_synth)
            try:
                assert rank_plans.path_sha256(be.path) == g["path_sha256"], f"{label}: bench builds another path than the fixture pins"
                assert be.n_slots == 4 and be.args.batch == bench.CONFIGS[config][3]
                if fe == "auto":
                    used = _pipelined(be, ctx, want, label)
                    print(f"{label}: front ends used {sorted(set(used))}")
                else:
                    _forced(dg, be, ctx, fe, want, label)
                if fe == "segs":
                    print(f"{label}: redone_frames {ctx.fallbacks()['redone_frames']}")
                if fe == "device" and n == 0 and config in OTHER_XCD_MAPPING:
                    monkeypatch.setenv("DOOMGPU_FRAME_PER_XCD", OTHER_XCD_MAPPING[config])     # (read by every launch)
                    _forced(dg, be, ctx, fe, want, f"{label}, DOOMGPU_FRAME_PER_XCD={OTHER_XCD_MAPPING[config]}")
                    monkeypatch.delenv("DOOMGPU_FRAME_PER_XCD")
            finally:
                ctx.close()
                be.scene.close()
    print(f"config {config}: {len(plans)} plan(s) in {time.time() - t0:.1f} s")
