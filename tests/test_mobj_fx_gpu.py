"""GPU tier of the map-object state machine (dg_scene_set_mobj_thinkers, DG_MOBJ_THINKERS): every frame a batch renders with the setting
on at its own timestamp equals the oracle's frame of the same WAD with set_mobj_state applied for the model's states at that timestamp
(tests/mobj_fx.py Sim), through every front end, at 320x200, 1280x800 and an odd size.  Each batch is one path with 72 distinct
timestamps that span dozens of state switches and three events (kill at tic 140, respawn at 300, explode at 500), plus far out,
saturation, +inf, NaN, -0.0 and negative time.  The oracle's frames with the model's states differ from its frames in spawn states for
more than half of the timestamps (asserted), so the comparison sees the animation.  Also: per-view overrides win over the thinkers,
the wall and light effects on as well, flags 0, the setting taking effect at upload, prepared slots replayed, the seg walk without
extra fallbacks, and frames redone on the host after a column overflow."""
import numpy as np
import pytest

import light_fx as lf
import mobj_fx as mf
import wall_fx as wf

pytestmark = pytest.mark.gpu

N = 72                                                    # >= 64: DG_FE_AUTO may pick the device seg walk
SIZES = [(320, 200), (1280, 800), (641, 401)]
FRONT_ENDS = [1, 2, 3, 0]                                 # DG_FE_HOST, DG_FE_DEVICE, DG_FE_DEVICE_SEGS, DG_FE_AUTO
EVENTS = [(mf.KILL, 140), (mf.RESPAWN, 300), (mf.EXPLODE, 500)]
SEED = 0x5EED


def _times():
    f = lambda v: float(np.float32(v))                    # noqa: E731
    t = [-0.0, -1.0, float("nan"), float("inf"), 1e5, 1e7, f(2.0 ** 32 / 35.0), 1e12]
    t += [mf.ts(T) for T in (1, 5, 6, 7, 10, 13, 17, 139, 140, 141, 148, 299, 300, 301, 499, 500, 502, 504)]
    t += [f(v) for v in np.linspace(0.37, 19.3, N - len(t))]
    assert len({repr(v) for v in t}) == N
    return t


TIMES = _times()
# Frames of path 1993, chosen with the oracle: 58 that show an object the thinkers drive and 14 that show none, so that the oracle's
# frames with the model's states differ from its spawn-state frames at 55 of the 72 timestamps (_share, asserted below).
IDX = [0, 26, 46, 54, 57, 94, 109, 140, 148, 158, 166, 174, 192, 206, 218, 229, 239, 266, 280, 294, 304, 314, 323, 332, 340, 360, 373, 381,
       391, 404, 431, 439, 448, 458, 466, 482, 497, 529, 535, 541, 550, 589, 603, 608, 629, 637, 660, 675, 684, 694, 703, 714, 722, 731, 741,
       749, 774, 793, 801, 806, 834, 853, 861, 871, 879, 887, 924, 933, 944, 963, 987, 999]
assert len(IDX) == N


@pytest.fixture(scope="module")
def wad():
    return mf.fx_wad()


@pytest.fixture(scope="module")
def sim(wad):
    return mf.Sim(wad, events=EVENTS)


def _fx_scene(dg, wad):
    sc = dg.Scene(wad, "E1M1")
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    for what, E in EVENTS:
        sc.mobj_event(what, mf.ts(E))
    return sc


@pytest.fixture(scope="module")
def fx_scene(dg, wad):
    sc = _fx_scene(dg, wad)
    yield sc
    sc.close()


def _views(dg, path):
    views = dg.make_views(path[IDX])
    for k, t in enumerate(TIMES):
        views[k].timestamp = t
    return views


def _set_states(osc, shown):
    """shown: the model's list, or {mobj: state}."""
    for i, s in (shown.items() if isinstance(shown, dict) else enumerate(shown)):
        if s == "null":
            osc.set_mobj_state(i, None)
        elif s is not None:
            osc.set_mobj_state(i, s[0], s[1], bool(s[2]))


def _oracle_frames(oracle, wad, path, W, H, sim=None, mobjs=None, light_seed=None, wall_flags=0, lights=None):
    """The oracle's frame k of `wad` (baked for the wall effects at t_k when wall_flags; sectors at the light model's levels at t_k when
    light_seed is given) with every driven map object in the model's state at t_k (sim) or all in spawn state, then the view's own
    entries `lights[k]` = [(sector, level)] and `mobjs[k]` = [(mobj, shown)] on top."""
    out = np.empty((N, H, W, 3), dtype=np.uint8)
    groups = {}
    for k, t in enumerate(TIMES):
        groups.setdefault(wf.bake_key(t, wall_flags) if wall_flags else 0, []).append(k)
    for ks in groups.values():
        baked = wf.bake(wad, TIMES[ks[0]], wall_flags) if wall_flags else wad
        for k in ks:
            osc = oracle.Scene(baked, "e1m1")               # a fresh scene per frame: overrides of the frame before must not stay
            if light_seed is not None:
                for s, l in enumerate(lf.levels_at(wad, light_seed, TIMES[k])):
                    osc.set_sector_light(s, l)
            for s, l in (lights[k] if lights is not None else []):
                osc.set_sector_light(s, l)
            if sim is not None:
                _set_states(osc, sim.shown(mf.tics(TIMES[k])))
            for i, s in (mobjs[k] if mobjs is not None else []):
                _set_states(osc, {i: s})
            out[k] = np.frombuffer(osc.render(W, H, list(path[IDX[k]]) + [TIMES[k]]), dtype=np.uint8).reshape(H, W, 3)
            osc.close()
    return out


@pytest.fixture(scope="module")
def oracle_frames(oracle, wad, sim, path1993):
    cache = {}

    def get(W, H, animated=True):
        if (W, H, animated) not in cache:
            cache[(W, H, animated)] = _oracle_frames(oracle, wad, path1993, W, H, sim=sim if animated else None)
        return cache[(W, H, animated)]
    return get


def _assert_frames(out, want, what):
    bad = [k for k in range(N) if not np.array_equal(out[k], want[k])]
    assert not bad, (what, bad[:8], [TIMES[k] for k in bad[:8]])


def _share(oracle_frames, W, H):
    a, b = oracle_frames(W, H), oracle_frames(W, H, animated=False)
    return sum(not np.array_equal(a[k], b[k]) for k in range(N))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fe", FRONT_ENDS)
def test_every_front_end_equals_the_oracle_with_the_states(dg, fx_scene, oracle_frames, path1993, W, H, fe):
    assert 2 * _share(oracle_frames, W, H) >= N           # the animation is in at least half of the frames compared
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render(_views(dg, path1993))
    _assert_frames(out, oracle_frames(W, H), (W, H, fe))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == 3 and ctx.fallbacks()["front_end"] == 0
    ctx.close()


def test_plain_frames_differ_from_the_animated_frames(dg, wad, oracle_frames, path1993):
    """(the comparison above is not vacuous: without the setting half of these frames or more differ)"""
    sc = dg.Scene(wad, "E1M1")
    ctx = dg.Context(320, 200, max_batch=N, slots=1, front_end=3)
    ctx.upload_scene(sc)
    out = ctx.render(_views(dg, path1993))
    want = oracle_frames(320, 200)
    assert 2 * sum(not np.array_equal(out[k], want[k]) for k in range(N)) >= N
    _assert_frames(out, oracle_frames(320, 200, animated=False), "spawn view")
    ctx.close()
    sc.close()


@pytest.mark.parametrize("fe", [1, 2, 3])
def test_view_state_wins_over_the_thinkers(dg, oracle, wad, sim, fx_scene, path1993, fe):
    """Every other view overrides some driven objects (and one the thinkers do not drive); the override wins, the rest keep their
    thinker's state."""
    W, H = 320, 200
    driven = [i for i, d in enumerate(sim.driven) if d]
    static = sim.driven.index(False)
    choices = [("TROO", 2, 1), ("BAR1", 1, 0), "null", ("POSS", 3, 0), ("CAND", 0, 1)]
    rng = np.random.default_rng(11)
    mobjs = [[(i, choices[int(rng.integers(len(choices)))]) for i in driven[k % 3::3]] + [(static, ("BON1", 1, 1))] if k % 2 else [] for k in range(N)]
    handle = lambda s: (-1, 0) if s == "null" else (fx_scene.sprite_frame(s[0], s[1]), s[2])   # noqa: E731
    states, keep = dg.make_view_states([([], [(i,) + handle(s) for i, s in m]) for m in mobjs])
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(fx_scene)
    out = ctx.render_state(_views(dg, path1993), states)
    _assert_frames(out, _oracle_frames(oracle, wad, path1993, W, H, sim=sim, mobjs=mobjs), ("view state", fe))
    ctx.close()
    del keep


ALL_WALLS = wf.ANIMATE | wf.SCROLL


@pytest.fixture(scope="module")
def allfx(oracle, path1993):
    """The WAD with all three test patches, and the oracle's frames for it: every effect on, and the same with one light and one
    map-object entry per view on top."""
    W, H = 320, 200
    wad = mf.fx_wad(lf.fx_wad(wf.fx_wad()))
    sim = mf.Sim(wad, events=EVENTS)
    plain = _oracle_frames(oracle, wad, path1993, W, H, sim=sim, light_seed=SEED, wall_flags=ALL_WALLS)
    over = _oracle_frames(oracle, wad, path1993, W, H, sim=sim, light_seed=SEED, wall_flags=ALL_WALLS, lights=[[(33, 64)]] * N, mobjs=[[(0, "null")]] * N)
    return wad, plain, over


@pytest.mark.parametrize("fe", [1, 2, 3])
def test_with_the_wall_and_light_effects_too(dg, allfx, path1993, fe):
    W, H = 320, 200
    wad, plain, over = allfx
    sc = _fx_scene(dg, wad)
    sc.set_wall_effects(ALL_WALLS)
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(sc)
    _assert_frames(ctx.render(_views(dg, path1993)), plain, ("walls and lights too", fe))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == 3
    # ... and with per-view light and map-object entries, which takes dg_light_rows and dg_mobj_rows through their in-place layout
    states, keep = dg.make_view_states([([(33, 64)], [(0, -1, 0)]) for _ in range(N)])
    _assert_frames(ctx.render_state(_views(dg, path1993), states), over, ("walls, lights and view states", fe))
    ctx.close()
    sc.close()
    del keep


def test_flags_zero_matches_the_plain_oracle(dg, wad, oracle_frames, path1993):
    W, H = 320, 200
    sc = _fx_scene(dg, wad)
    sc.set_mobj_thinkers(0)
    for fe in FRONT_ENDS:
        ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(W, H, animated=False), ("flags 0", fe))
        ctx.close()
    sc.close()


def test_the_setting_takes_effect_at_upload(dg, wad, oracle_frames, path1993):
    """A ctx draws with the tables and events of its last dg_upload_scene: events added or the setting cleared after the upload do
    nothing to it until the next one."""
    W, H = 320, 200
    for fe in (1, 2, 3):
        sc = _fx_scene(dg, wad)
        ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
        ctx.upload_scene(sc)
        sc.mobj_event(mf.KILL, mf.ts(600))
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(W, H), ("event after upload", fe))
        sc.set_mobj_thinkers(0)
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(W, H), ("cleared after upload", fe))
        ctx.upload_scene(sc)
        _assert_frames(ctx.render(_views(dg, path1993)), oracle_frames(W, H, animated=False), ("cleared and uploaded", fe))
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


def test_redone_frames_keep_the_uploaded_thinkers(dg, wad, sim, oracle_frames, path1993, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=5 makes DG_FE_DEVICE redo frames on the host at dg_wait.  The scene moves on between submit and wait
    (a state set on a driven object and on one that is not, the setting cleared): the redone frames still show the submit-time scene
    with the thinkers the ctx uploaded."""
    W, H = 1280, 800
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "5")
    sc = _fx_scene(dg, wad)
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=2)
    ctx.upload_scene(sc)
    ctx.submit(0, _views(dg, path1993))
    sc.set_mobj_state(sim.driven.index(True), None)
    sc.set_mobj_state(sim.driven.index(False), "CAND", 1, True)
    sc.set_mobj_thinkers(0)
    ctx.wait(0)
    _assert_frames(ctx.readback(0, 0, N), oracle_frames(W, H), "redone")
    assert ctx.fallbacks()["redone_frames"] > 0
    ctx.close()
    sc.close()
