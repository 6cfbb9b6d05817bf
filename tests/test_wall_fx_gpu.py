"""GPU tier of the wall effects (dg_scene_set_wall_effects): every frame a batch renders with DG_WALL_ANIMATE | DG_WALL_SCROLL at its own
timestamp equals the oracle's frame of the baked WAD at that timestamp (tests/wall_fx.py bake), through every front end, at 320x200,
1280x800 and an odd width.  Each batch is one path with 72 distinct timestamps, up to past the tic count at which k * tics wraps 2^16 for
k = 1 and 2.  Also: per-view sector lights, prepared slots replayed, flags 0 on the same WAD, and no more host fallbacks than flags 0."""
import numpy as np
import pytest

import wall_fx as wf

pytestmark = pytest.mark.gpu

N = 72                                                    # >= 64: DG_FE_AUTO may pick the device seg walk
SIZES = [(320, 200), (1280, 800), (641, 401)]
FRONT_ENDS = [1, 2, 3, 0]                                 # DG_FE_HOST, DG_FE_DEVICE, DG_FE_DEVICE_SEGS, DG_FE_AUTO


def _times():
    """N distinct timestamps: the 1/3 s frame edges, then 0 .. 2400 s — past 65536 / 35 (k = 1 wraps) and 32768 / 35 (k = 2)."""
    t = [0.0, 0.2, float(np.float32(1 / 3)), 0.7, 1.0, 1.4]
    t += [float(np.float32(v)) for v in np.linspace(3.0, 2400.0, N - len(t) - 4)]
    t += [float(np.float32(65536 / 35)), float(np.nextafter(np.float32(65536 / 35), np.float32(0))), 936.3, 1872.6]
    assert len(set(t)) == N
    return t


TIMES = _times()
IDX = [int(i) for i in np.linspace(0, 999, N)]


@pytest.fixture(scope="module")
def wad():
    return wf.fx_wad()


@pytest.fixture(scope="module")
def fx_scene(dg, wad):
    sc = dg.Scene(wad, "E1M1")
    sc.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
    yield sc
    sc.close()


def _views(dg, path):
    views = dg.make_views(path[IDX])
    for k, t in enumerate(TIMES):
        views[k].timestamp = t
    return views


def _oracle_frames(oracle, wad, path, W, H, lights=None, flags=wf.ANIMATE | wf.SCROLL):
    """The oracle's frame of bake(wad, t_k) for every view k; one oracle scene per bake key."""
    groups = {}
    for k, t in enumerate(TIMES):
        groups.setdefault(wf.bake_key(t, flags), []).append(k)
    out = np.empty((N, H, W, 3), dtype=np.uint8)
    for ks in groups.values():
        osc = oracle.Scene(wf.bake(wad, TIMES[ks[0]], flags) if flags else wad, "e1m1")
        for k in ks:
            if lights is not None:
                for s, l in lights[k]:
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


def test_bake_keys_cover_the_wrap():
    assert len({wf.bake_key(t) for t in TIMES}) >= 40
    assert max(wf.tics(t) for t in TIMES) * 1 >= 65536 and any(2 * wf.tics(t) >= 65536 > wf.tics(t) for t in TIMES)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fe", FRONT_ENDS)
def test_every_front_end_equals_the_baked_oracle(dg, fx_scene, oracle_frames, path1993, W, H, fe):
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render(_views(dg, path1993))
    _assert_frames(out, oracle_frames(W, H), (W, H, fe))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == 3 and ctx.fallbacks()["front_end"] == 0
    ctx.close()


def test_plain_frames_differ_from_the_baked_ones(dg, wad, oracle_frames, path1993):
    """(the comparison above is not vacuous: without the effects most of these frames differ)"""
    sc = dg.Scene(wad, "E1M1")
    ctx = dg.Context(320, 200, max_batch=N, slots=1, front_end=3)
    ctx.upload_scene(sc)
    out = ctx.render(_views(dg, path1993))
    want = oracle_frames(320, 200)
    assert sum(not np.array_equal(out[k], want[k]) for k in range(N)) >= N // 2
    ctx.close()
    sc.close()


@pytest.mark.parametrize("fe", [1, 3])
def test_per_view_sector_lights(dg, oracle, wad, fx_scene, path1993, fe):
    W, H = 320, 200
    rng = np.random.default_rng(7)
    n_sec = fx_scene.sector_count()
    lights = [[(s, int(rng.choice([0, 64, 128, 200, 255]))) for s in range(n_sec)] for _ in range(N)]
    states, keep = dg.make_view_states([(l, []) for l in lights])
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render_state(_views(dg, path1993), states)
    _assert_frames(out, _oracle_frames(oracle, wad, path1993, W, H, lights=lights), ("lights", fe))
    ctx.close()
    del keep


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


def test_flags_zero_matches_the_unbaked_oracle(dg, oracle, wad, path1993):
    W, H = 320, 200
    sc = dg.Scene(wad, "E1M1")
    sc.set_wall_effects(3)
    sc.set_wall_effects(0)
    want = _oracle_frames(oracle, wad, path1993, W, H, flags=0)
    for fe in FRONT_ENDS:
        ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        _assert_frames(ctx.render(_views(dg, path1993)), want, ("flags 0", fe))
        ctx.close()
    sc.close()


def test_flags_take_effect_at_upload(dg, wad, fx_scene, oracle_frames, path1993):
    """Clearing the flags after dg_upload_scene leaves the ctx drawing with the effects it uploaded."""
    sc = dg.Scene(wad, "E1M1")
    sc.set_wall_effects(3)
    for fe in (1, 3):
        ctx = dg.Context(320, 200, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        sc.set_wall_effects(0)
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(320, 200), ("after clear", fe))
        sc.set_wall_effects(3)
        ctx.close()
    sc.close()


def test_fallbacks_do_not_rise(dg, wad, fx_scene, path1993):
    plain = dg.Scene(wad, "E1M1")
    counts = []
    for sc in (plain, fx_scene):
        ctx = dg.Context(1280, 800, max_batch=N, slots=1, front_end=3)
        ctx.upload_scene(sc)
        for _ in range(3):
            ctx.render(_views(dg, path1993))
        counts.append(ctx.fallbacks())
        ctx.close()
    assert counts[1]["front_end"] <= counts[0]["front_end"] and counts[1]["redone_frames"] <= counts[0]["redone_frames"]
    plain.close()
