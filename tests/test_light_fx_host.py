"""CPU tier of the sector light effects (dg_scene_set_light_effects, DG_LIGHT_THINKERS): the model's shortcuts against its own literal
tic-by-tic run; dg_scene_sector_lights_at against the model at every tic up to 100 000, at f32 tic boundaries, far out, at saturation and
for NaN / -0.0 / negative time, for two seeds; which types depend on the seed; the host walker (dg_build_lists) with the effects on
against a flags-0 scene given the model's levels; flags 0 after 1; the error returns; dg_light_rows' ISA budget; and the wrapping glow
orbits at the ends of the i16 range."""
import os

import numpy as np
import pytest

import light_fx as lf

F32 = np.float32
SEEDS = (0, 0x0123456789ABCDEF)
VIEWS = list(range(0, 1000, 83))


@pytest.fixture(scope="module")
def wad():
    return lf.fx_wad()


@pytest.fixture(scope="module")
def models(wad):
    return {s: lf.model(wad, s) for s in SEEDS}


def _ts(T):
    """An f32 timestamp whose tic count is T."""
    t = F32((T + 0.5) / 35.0)
    assert lf.tics(t) == T
    return float(t)


def _scene(dg, wad, flags=lf.THINKERS, seed=0):
    sc = dg.Scene(wad, "E1M1")
    sc.set_light_effects(flags, seed)
    return sc


def _rec_levels(m, got):
    return [int(got[r[0]]) for r in m.recs]


def test_fixture_wad_has_what_the_contract_names(wad, models):
    m = models[0]
    types = {t for _, t, _, _ in m.recs}
    assert types == set(lf.TYPES)
    assert lf.sectors(wad)[39][1] == 9 and 39 not in m.index                    # a special with no thinker
    assert any(t == 17 and mn > mx for _, t, mn, mx in m.recs)                   # fire: min above max
    for s, t in ((36, 1), (15, 2)):                                              # flash and strobe with no darker neighbour
        assert lf.min_surrounding(wad, s) == lf.sectors(wad)[s][0] and lf.sectors(wad)[s][1] == t
    levels = {l for l, _ in lf.sectors(wad)}
    assert {0, 255}.issubset(levels) and any(l < 0 for l in levels) and any(l > 255 for l in levels)


def test_model_shortcuts_equal_its_literal_run(models):
    for m in models.values():
        longest = max(m._short[i][-1] for i, r in enumerate(m.recs) if r[1] == 1)
        n = 2 * longest + 100
        lit = m.literal(n)
        for i in range(len(m.recs)):
            short = np.array([m.level(i, T) for T in range(n + 1)])
            assert np.array_equal(short, lit[:, i]), (m.recs[i], int(np.argmax(short != lit[:, i])))


@pytest.mark.parametrize("seed", SEEDS)
def test_sector_lights_at_every_tic(dg, wad, models, seed):
    m = models[seed]
    lit = m.literal(100_000)
    sc = _scene(dg, wad, seed=seed)
    base = np.array(m.base, dtype=np.int16)
    others = np.ones(len(base), dtype=bool)
    others[[r[0] for r in m.recs]] = False
    for T in range(100_001):
        got = sc.sector_lights_at(_ts(T))
        assert _rec_levels(m, got) == lit[T].tolist(), T
        assert np.array_equal(got[others], base[others]), T
    sc.close()


def _boundaries():
    out = []
    for T in (1, 2, 4, 5, 20, 35, 36, 41, 4095 * 4, 4096 * 4, 65536, 74_000, 1 << 20, 1 << 24, 12_345_678, (1 << 32) - 1000):
        t = F32(T / 35.0)
        while lf.tics(t) >= T:
            t = np.nextafter(t, F32(-1))
        while lf.tics(t) < T:
            t = np.nextafter(t, F32(np.inf))
        out += [float(np.nextafter(t, F32(-1))), float(t)]                       # the last f32 before tic T and the first of it
    return out


SPECIAL_TIMES = [1e5, 1e7, float(F32(2.0 ** 32 / 35.0)), 2.0 ** 32 / 35.0 * 1.01, 1e12, float("inf"), float("nan"), -0.0, -1.0, -1e30,
                 float("-inf")]


@pytest.mark.parametrize("seed", SEEDS)
def test_sector_lights_at_boundaries_far_out_and_saturation(dg, wad, models, seed):
    m = models[seed]
    sc = _scene(dg, wad, seed=seed)
    for t in _boundaries() + SPECIAL_TIMES:
        got = sc.sector_lights_at(t)
        assert got.tolist() == m.levels(lf.tics(t)), t
    assert lf.tics(float("inf")) == (1 << 32) - 1 and lf.tics(float("nan")) == 0 and lf.tics(-0.0) == 0
    assert sc.sector_lights_at(float("nan")).tolist() == sc.sector_lights_at(0.0).tolist()
    sc.close()


def test_seed_dependence(wad, models):
    """8, 12, 13 never depend on the seed; 1, 2, 3, 4, 17 do (a strobe's phase is one of 8, so two seeds may share it: five are tried)."""
    runs = [models[s].literal(20_000) for s in SEEDS] + [lf.Model(wad, s).literal(20_000) for s in (1, 2, 3)]
    for i, (s, t, mn, mx) in enumerate(models[SEEDS[0]].recs):
        same = all(np.array_equal(runs[0][:, i], r[:, i]) for r in runs[1:])
        assert same == (t in (8, 12, 13) or mn == mx), (s, t)


def test_scene_level_rules_without_an_effect(dg, wad):
    """set_sector_light reaches only sectors without an effect; flags 0 gives the scene's levels."""
    sc = _scene(dg, wad)
    m = lf.model(wad, 0)
    sc.set_sector_light(6, 17)                                                   # a flash sector: the effect wins
    sc.set_sector_light(39, 18)                                                  # special 9: no thinker
    got = sc.sector_lights_at(_ts(1000))
    assert got[39] == 18 and got[6] == m.level(m.index[6], 1000)
    sc.set_light_effects(0)
    got = sc.sector_lights_at(_ts(1000))
    assert got[6] == 17 and got[39] == 18 and got[43] == lf.sectors(wad)[43][0]
    sc.close()


def _records(fl):
    rs = [tuple(getattr(r, f) for f, _ in r._fields_) for r in fl.renders[:fl.n_renders]]
    cols = [tuple(getattr(c, f) for f, _ in c._fields_) for c in fl.columns[:fl.n_columns]]
    vps = [tuple(getattr(v, f) for f, _ in v._fields_) for v in fl.visplanes[:fl.n_visplanes]]
    return rs, cols, vps, list(fl.plane_tb[:fl.n_plane_tb]), [(o.kind, o.index) for o in fl.order[:fl.n_order]]


@pytest.mark.parametrize("seed", SEEDS)
def test_host_walker_equals_the_levels_applied(dg, wad, path1993, seed):
    sc = _scene(dg, wad, seed=seed)
    plain = dg.Scene(wad, "E1M1")
    changed = 0
    for j, t in enumerate([0.0, 0.4, 3.3, 17.0, 123.4, 2400.0, 1e5, 1e7, float("inf"), float("nan"), -2.0]):
        levels = lf.levels_at(wad, seed, t)
        for s, l in enumerate(levels):
            plain.set_sector_light(s, l)
        views = dg.make_views(path1993[VIEWS], timestamp=t)
        for k in range(len(VIEWS)):
            got = _records(sc.build_lists(320, 200, views[k]))
            assert got == _records(plain.build_lists(320, 200, views[k])), (t, k)
            if j == 3:
                fresh = dg.Scene(wad, "E1M1")
                changed += got != _records(fresh.build_lists(320, 200, views[k]))
                fresh.close()
    assert changed >= 4                                                          # the effects do reach these views
    plain.close()
    sc.close()


def test_flags_zero_lists_are_unchanged(dg, wad, path1993):
    a = dg.Scene(wad, "E1M1")
    b = dg.Scene(wad, "E1M1")
    b.set_light_effects(lf.THINKERS, 7)
    b.set_light_effects(0, 7)
    views = dg.make_views(path1993[VIEWS], timestamp=17.0)
    for k in range(len(VIEWS)):
        assert _records(a.build_lists(320, 200, views[k])) == _records(b.build_lists(320, 200, views[k])), k
    a.close()
    b.close()


def test_error_returns(dg, wad):
    import ctypes
    L = dg.lib()
    sc = dg.Scene(wad, "E1M1")
    for bad in (2, 4, 0x80000000, 0xFFFFFFFF):
        assert L.dg_scene_set_light_effects(sc._h, bad, 0) == dg.DG_ERR_INVALID
    assert L.dg_scene_set_light_effects(None, 1, 0) == dg.DG_ERR_INVALID
    n = sc.sector_count()
    buf = (ctypes.c_int16 * (n + 1))()
    for bad_n in (n - 1, n + 1, 0, -1):
        assert L.dg_scene_sector_lights_at(sc._h, 1.0, buf, bad_n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_lights_at(None, 1.0, buf, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_lights_at(sc._h, 1.0, None, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_set_light_effects(sc._h, 1, 2 ** 64 - 1) == dg.DG_OK
    assert L.dg_scene_sector_lights_at(sc._h, 1.0, buf, n) == dg.DG_OK
    sc.close()


@pytest.mark.parametrize("level, neighbours", [(32765, 32767), (32760, 32767), (-32765, -32768), (-32765, None), (-32761, -32768),
                                               (-32768, None), (200, 199), (200, 192), (200, 191), (200, 183)])
def test_glow_at_the_ends_of_the_i16_range(dg, wad, level, neighbours):
    """The glow recurrence where its tests wrap: one glow sector at `level`, its neighbours at `neighbours` (None: at `level` too)."""
    s = 43
    nb = {b for f, b in lf.two_sided_pairs(wad) if f == s} | {f for f, b in lf.two_sided_pairs(wad) if b == s}
    nb.discard(s)
    w = lf.set_sectors(wad, {s: (8, level), **{n: (0, level if neighbours is None else neighbours) for n in nb}})
    m = lf.Model(w, 0)
    i = m.index[s]
    lit = m.literal(3 * 8192 + 50)[:, i]
    sc = _scene(dg, w)
    for T in list(range(0, len(lit), 3)) + [len(lit) - 1]:
        assert sc.sector_lights_at(_ts(T))[s] == lit[T], (T, int(lit[T]))
    t = 1e9 / 35.0
    assert sc.sector_lights_at(t)[s] == m.level(i, lf.tics(t))
    sc.close()


def test_light_rows_kernel_has_no_lds_and_no_scratch():
    from test_wall_fx_isa import _kernels
    ks = _kernels("light_fx_kernels.hip")
    hits = [(n, v) for n, v in ks.items() if "dg_light_rows" in n]
    assert len(hits) == 1, list(ks)
    name, (lds, scratch, vgpr) = hits[0]
    assert lds == 0 and scratch == 0 and vgpr <= 64, (name, lds, scratch, vgpr)


def test_light_rows_kernel_is_built_into_the_library(dg):
    mk = open(os.path.join(os.path.dirname(dg.LIB_PATH), "csrc", "Makefile")).read()
    assert "light_fx_kernels.hip" in mk
