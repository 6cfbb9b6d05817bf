"""GPU tier of the sector light effects (dg_scene_set_light_effects, DG_LIGHT_THINKERS): every frame a batch renders with the effects on
at its own timestamp equals the oracle's frame of the same WAD with set_sector_light applied for the model's levels at that timestamp
(tests/light_fx.py levels_at), through every front end, at 320x200, 1280x800 and an odd size.  Each batch is one path with 72 distinct
timestamps: the strobes' first switches, the flash period, far out, saturation, +inf, NaN, -0.0 and negative time.  Also: per-view
overrides win over the effects, the wall effects on as well, flags 0, the flags taking effect at upload, prepared slots replayed, the seg
walk without extra fallbacks, and frames redone on the host after a column overflow."""
import numpy as np
import pytest

import light_fx as lf
import wall_fx as wf

pytestmark = pytest.mark.gpu

N = 72                                                    # >= 64: DG_FE_AUTO may pick the device seg walk
SIZES = [(320, 200), (1280, 800), (641, 401)]
FRONT_ENDS = [1, 2, 3, 0]                                 # DG_FE_HOST, DG_FE_DEVICE, DG_FE_DEVICE_SEGS, DG_FE_AUTO
SEED = 0x5EED


def _times():
    f = lambda v: float(np.float32(v))                    # noqa: E731
    t = [-0.0, -1.0, float("nan"), float("inf"), 1e5, 1e7, f(2.0 ** 32 / 35.0), 1e12]
    t += [f((T + 0.5) / 35.0) for T in (1, 2, 3, 5, 8, 9, 15, 16, 20, 21, 36, 41, 60, 61, 64, 65)]
    t += [f(v) for v in (2136.0, 2137.5, 2140.0, 2200.0, 2400.0)]
    t += [f(v) for v in np.linspace(2.0, 2000.0, N - len(t))]
    assert len({repr(v) for v in t}) == N
    return t


TIMES = _times()
IDX = [int(i) for i in np.linspace(0, 999, N)]


@pytest.fixture(scope="module")
def wad():
    return lf.fx_wad()


@pytest.fixture(scope="module")
def fx_scene(dg, wad):
    sc = dg.Scene(wad, "E1M1")
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    yield sc
    sc.close()


def _views(dg, path):
    views = dg.make_views(path[IDX])
    for k, t in enumerate(TIMES):
        views[k].timestamp = t
    return views


def _oracle_frames(oracle, wad, path, W, H, lights=None, effects=True, wall_flags=0):
    """The oracle's frame k of `wad` (baked for the wall effects at t_k when wall_flags) with every sector at the model's level at t_k
    (effects) or the WAD's, then the view's own entries `lights[k]` on top."""
    out = np.empty((N, H, W, 3), dtype=np.uint8)
    groups = {}
    for k, t in enumerate(TIMES):
        groups.setdefault(wf.bake_key(t, wall_flags) if wall_flags else 0, []).append(k)
    base = [l for l, _ in lf.sectors(wad)]
    for ks in groups.values():
        osc = oracle.Scene(wf.bake(wad, TIMES[ks[0]], wall_flags) if wall_flags else wad, "e1m1")
        for k in ks:
            levels = lf.levels_at(wad, SEED, TIMES[k]) if effects else base
            for s, l in enumerate(levels):
                osc.set_sector_light(s, l)
            for s, l in (lights[k] if lights is not None else []):
                osc.set_sector_light(s, l)
            out[k] = np.frombuffer(osc.render(W, H, list(path[IDX[k]]) + [TIMES[k]]), dtype=np.uint8).reshape(H, W, 3)
        osc.close()
    return out


@pytest.fixture(scope="module")
def oracle_frames(oracle, wad, path1993):
    cache = {}

    def get(W, H):
        if (W, H) not in cache:
            cache[(W, H)] = _oracle_frames(oracle, wad, path1993, W, H)
        return cache[(W, H)]
    return get


def _assert_frames(out, want, what):
    bad = [k for k in range(N) if not np.array_equal(out[k], want[k])]
    assert not bad, (what, bad[:8], [TIMES[k] for k in bad[:8]])


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fe", FRONT_ENDS)
def test_every_front_end_equals_the_oracle_with_the_levels(dg, fx_scene, oracle_frames, path1993, W, H, fe):
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render(_views(dg, path1993))
    _assert_frames(out, oracle_frames(W, H), (W, H, fe))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == 3 and ctx.fallbacks()["front_end"] == 0
    ctx.close()


def test_plain_frames_differ_from_the_effect_frames(dg, wad, oracle_frames, path1993):
    """(the comparison above is not vacuous: without the effects a quarter of these frames or more differ)"""
    sc = dg.Scene(wad, "E1M1")
    ctx = dg.Context(320, 200, max_batch=N, slots=1, front_end=3)
    ctx.upload_scene(sc)
    out = ctx.render(_views(dg, path1993))
    want = oracle_frames(320, 200)
    assert sum(not np.array_equal(out[k], want[k]) for k in range(N)) >= N // 4
    ctx.close()
    sc.close()


@pytest.mark.parametrize("fe", [1, 2, 3])
def test_view_state_wins_over_the_effects(dg, oracle, wad, fx_scene, path1993, fe):
    """Every other view overrides some effect sectors (and one plain sector); the override wins, the rest keep their effects."""
    W, H = 320, 200
    m = lf.model(wad, SEED)
    fx_sectors = [r[0] for r in m.recs]
    rng = np.random.default_rng(11)
    lights = [[(s, int(rng.choice([0, 40, 128, 200, 255]))) for s in fx_sectors[k % 3::3]] + [(33, 64)] if k % 2 else [] for k in range(N)]
    states, keep = dg.make_view_states([(l, []) for l in lights])
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render_state(_views(dg, path1993), states)
    _assert_frames(out, _oracle_frames(oracle, wad, path1993, W, H, lights=lights), ("view state", fe))
    ctx.close()
    del keep


@pytest.mark.parametrize("fe", [1, 2, 3])
def test_with_the_wall_effects_too(dg, oracle, path1993, fe):
    W, H = 320, 200
    both = lf.fx_wad(wf.fx_wad())
    sc = dg.Scene(both, "E1M1")
    sc.set_wall_effects(wf.ANIMATE | wf.SCROLL)
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(sc)
    out = ctx.render(_views(dg, path1993))
    _assert_frames(out, _oracle_frames(oracle, both, path1993, W, H, wall_flags=wf.ANIMATE | wf.SCROLL), ("walls too", fe))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == 3
    ctx.close()
    sc.close()


def test_flags_zero_matches_the_plain_oracle(dg, oracle, wad, path1993):
    W, H = 320, 200
    sc = dg.Scene(wad, "E1M1")
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    sc.set_light_effects(0)
    want = _oracle_frames(oracle, wad, path1993, W, H, effects=False)
    for fe in FRONT_ENDS:
        ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        _assert_frames(ctx.render(_views(dg, path1993)), want, ("flags 0", fe))
        ctx.close()
    sc.close()


def test_flags_take_effect_at_upload(dg, oracle, wad, oracle_frames, path1993):
    """A ctx draws with the flags of its last dg_upload_scene: set after the upload they do nothing until the next one; cleared after
    it, the ctx keeps drawing the effects."""
    W, H = 320, 200
    plain = _oracle_frames(oracle, wad, path1993, W, H, effects=False)
    for fe in (1, 2, 3):
        sc = dg.Scene(wad, "E1M1")
        ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
        _assert_frames(ctx.render(_views(dg, path1993)), plain, ("set after upload", fe))
        ctx.upload_scene(sc)
        sc.set_light_effects(0)
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(W, H), ("cleared after upload", fe))
        ctx.close()
        sc.close()


@pytest.mark.parametrize("fe", [2, 3])
def test_prepared_slot_replays(dg, fx_scene, oracle_frames, path1993, fe):
    W, H = 320, 200
    ctx = dg.Context(W, H, max_batch=N, slots=2, front_end=fe)
    ctx.upload_scene(fx_scene)
    ctx.prepare(1, _views(dg, path1993))
    for _ in range(2):
        ctx.replay(1)
        ctx.wait(1)
        _assert_frames(ctx.readback(1, 0, N), oracle_frames(W, H), ("replay", fe))
    ctx.close()


def test_seg_walk_keeps_its_path_and_fallbacks(dg, wad, fx_scene, path1993):
    plain = dg.Scene(wad, "E1M1")
    counts = []
    for sc in (plain, fx_scene):
        ctx = dg.Context(1280, 800, max_batch=N, slots=1, front_end=3)
        ctx.upload_scene(sc)
        for _ in range(3):
            ctx.render(_views(dg, path1993))
            assert ctx.timing(0)["front_end"] == 3
        counts.append(ctx.fallbacks())
        ctx.close()
    assert counts[1]["front_end"] <= counts[0]["front_end"] and counts[1]["redone_frames"] <= counts[0]["redone_frames"]
    plain.close()


def test_redone_frames_keep_the_uploaded_effects(dg, wad, oracle_frames, path1993, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=5 makes DG_FE_DEVICE redo frames on the host at dg_wait.  The scene moves on between submit and wait
    (a level set on an effect sector and on a plain one, the flags cleared): the redone frames still show the submit-time scene with
    the effects the ctx uploaded."""
    W, H = 1280, 800
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "5")
    sc = dg.Scene(wad, "E1M1")
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=2)
    ctx.upload_scene(sc)
    ctx.submit(0, _views(dg, path1993))
    sc.set_sector_light(6, 3)                             # a flash sector
    sc.set_sector_light(33, 3)                            # no effect
    sc.set_light_effects(0)
    ctx.wait(0)
    _assert_frames(ctx.readback(0, 0, N), oracle_frames(W, H), "redone")
    assert ctx.fallbacks()["redone_frames"] > 0
    ctx.close()
    sc.close()
