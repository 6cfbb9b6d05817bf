"""CPU tier of the wall effects (dg_scene_set_wall_effects, DG_WALL_ANIMATE / DG_WALL_SCROLL): the library's own list builder with the
effects on equals, record for record, its builder on the baked WAD (tests/wall_fx.py bake) over a grid of timestamps that covers the
1/3 s frame edges, the tic wrap at 65536 / 35 s, saturation, +inf, NaN and negative time; dg_scene_wall_texture_id against the Python
rule; flags 0 after 3; stable bitmap ids; the error returns."""
import struct

import numpy as np
import pytest

import wall_fx as wf

F32 = np.float32


def _ulp(x, d):
    return float(np.nextafter(F32(x), F32(d * np.inf)))


GRID = [0.0, _ulp(1 / 3, -1), float(F32(1 / 3)), _ulp(1 / 3, 1), 1.0, 7.3, _ulp(65536 / 35, -1), float(F32(65536 / 35)), _ulp(65536 / 35, 1),
        1e6, 1e12, float("inf"), float("nan"), -1.0]
VIEWS = list(range(0, 1000, 83))


@pytest.fixture(scope="module")
def wad():
    return wf.fx_wad()


@pytest.fixture(scope="module")
def plain(dg, wad):
    """The test WAD without effects, and its texture id -> name map."""
    sc = dg.Scene(wad, "E1M1")
    yield sc, _texture_ids(dg, sc, wf.texture_names(wad))
    sc.close()


def _texture_ids(dg, sc, names):
    return {i: n for n in names if (i := dg.lib().dg_scene_texture_id(sc._h, n.encode())) >= 0}


def _records(fl, names):
    """The lists of one frame as plain tuples; bitmap ids through `names` (texture ids -> name), other ids (sprites) kept as ('id', n)."""
    def bitmap(i):
        return names.get(i, ("id", i))
    rs = [(bitmap(r.bitmap),) + tuple(getattr(r, f) for f, _ in r._fields_[1:]) for r in fl.renders[:fl.n_renders]]
    cols = [tuple(getattr(c, f) for f, _ in c._fields_) for c in fl.columns[:fl.n_columns]]
    vps = [tuple(getattr(v, f) for f, _ in v._fields_) for v in fl.visplanes[:fl.n_visplanes]]
    tb = list(fl.plane_tb[:fl.n_plane_tb])
    order = [(o.kind, o.index) for o in fl.order[:fl.n_order]]
    return rs, cols, vps, tb, order


def _same_up_to_sprite_ids(a, b):
    """Equal, with sprite bitmap ids (not texture names) matched by a consistent one-to-one map between the two scenes."""
    m, inv = {}, {}
    assert len(a[0]) == len(b[0])
    for ra, rb in zip(a[0], b[0]):
        if isinstance(ra[0], tuple) and isinstance(rb[0], tuple):
            assert m.setdefault(ra[0], rb[0]) == rb[0] and inv.setdefault(rb[0], ra[0]) == ra[0]
            ra, rb = ra[1:], rb[1:]
        assert ra == rb
    assert a[1:] == b[1:]


def test_fixture_wad_has_what_the_contract_names(wad):
    have = wf.texture_names(wad)
    live = wf.live_lists(wad)
    assert [l[0] for l in live] == ["SLADRIP1", "FIREWALA", "FIREBLU1", "BFALL1"]
    assert "BLODGR3" in have and "BLODGR4" not in have                    # BLODGR1-3 present, its list dead
    k = wf.scroll_counts(wad)
    assert max(k) == 2 and sum(1 for v in k if v) >= 6
    lumps = {n: wad[o:o + s] for n, o, s in wf.synth.wad_directory(wad)}
    sides = lumps["SIDEDEFS"]
    assert any(k[s] and struct.unpack_from("<h", sides, 30 * s)[0] < -32700 for s in range(len(k)))
    named = [sides[30 * s + o:30 * s + o + 8].split(b"\0")[0].decode() for s in range(len(k)) for o in (4, 12, 20)]
    for n in ("SLADRIP2", "BFALL3", "FIREWALB", "FIREBLU2", "BLODGR2"):
        assert n in named, n


@pytest.mark.parametrize("flags", [wf.ANIMATE, wf.SCROLL, wf.ANIMATE | wf.SCROLL])
def test_lists_equal_the_baked_wad(dg, wad, plain, path1993, flags):
    sc = dg.Scene(wad, "E1M1")
    sc.set_wall_effects(flags)
    names = _texture_ids(dg, sc, wf.texture_names(wad))
    changed = 0
    for t in GRID:
        baked = wf.bake(wad, t, flags)
        bs = dg.Scene(baked, "E1M1")
        bnames = _texture_ids(dg, bs, wf.texture_names(baked))
        views = dg.make_views(path1993[VIEWS], timestamp=t)
        for k in range(len(VIEWS)):
            got = _records(sc.build_lists(320, 200, views[k]), names)
            want = _records(bs.build_lists(320, 200, views[k]), bnames)
            _same_up_to_sprite_ids(got, want)
            if t == 7.3:
                changed += got[0] != _records(plain[0].build_lists(320, 200, views[k]), plain[1])[0]
        bs.close()
    assert changed >= 3                                                   # the effects do reach these views
    sc.close()


def test_wall_texture_id_follows_the_rule(dg, wad):
    sc = dg.Scene(wad, "E1M1")
    L = dg.lib()
    for n in ("SLADRIP2", "BFALL1"):
        assert sc.wall_texture_id(n, 5.0) == L.dg_scene_texture_id(sc._h, n.encode())     # flags 0: no animation
    sc.set_wall_effects(dg.DG_WALL_ANIMATE)
    have = wf.texture_names(wad)
    for l in wf.WALL_LISTS:
        for n in l:
            for t in GRID:
                got = sc.wall_texture_id(n.lower() if n.endswith("2") else n, t)
                if n not in have:
                    assert got < 0, (n, t)
                    continue
                want = L.dg_scene_texture_id(sc._h, wf.wall_name(wad, n, t).encode())
                assert want >= 0 and got == want, (n, t, got, want)
    # the dead list stays static
    assert sc.wall_texture_id("BLODGR2", 1.0) == L.dg_scene_texture_id(sc._h, b"BLODGR2")
    assert sc.wall_texture_id("BRICK1", 1.0) == L.dg_scene_texture_id(sc._h, b"BRICK1")
    sc.set_wall_effects(dg.DG_WALL_SCROLL)
    assert sc.wall_texture_id("SLADRIP1", 1.0) == L.dg_scene_texture_id(sc._h, b"SLADRIP1")
    sc.close()


def test_flags_zero_after_three_is_never_set_and_ids_stay(dg, wad, path1993):
    L = dg.lib()
    plain = dg.Scene(wad, "E1M1")
    sc = dg.Scene(wad, "E1M1")
    names = sorted(wf.texture_names(wad))
    before = {n: L.dg_scene_texture_id(sc._h, n.encode()) for n in names}
    sc.set_wall_effects(3)
    after = {n: L.dg_scene_texture_id(sc._h, n.encode()) for n in names}
    assert all(after[n] == i for n, i in before.items() if i >= 0)         # new bitmaps are appended
    assert all(after[n] >= 0 for l in wf.live_lists(wad) for n in l)
    sc.set_wall_effects(0)
    views = dg.make_views(path1993[VIEWS], timestamp=7.3)
    for k in range(len(VIEWS)):
        a = _records(sc.build_lists(320, 200, views[k]), {})
        b = _records(plain.build_lists(320, 200, views[k]), {})
        assert a == b, k
    sc.close()
    plain.close()


def test_error_returns(dg, wad):
    L = dg.lib()
    sc = dg.Scene(wad, "E1M1")
    for bad in (4, 8, 0x80000000, 0xFFFFFFFF):
        assert L.dg_scene_set_wall_effects(sc._h, bad) == dg.DG_ERR_INVALID
    assert L.dg_scene_set_wall_effects(None, 1) == dg.DG_ERR_INVALID
    assert L.dg_scene_wall_texture_id(None, b"BFALL1", 0.0) == dg.DG_ERR_INVALID
    assert L.dg_scene_wall_texture_id(sc._h, None, 0.0) == dg.DG_ERR_INVALID
    assert L.dg_scene_set_wall_effects(sc._h, 3) == dg.DG_OK
    sc.close()


def test_version_is_release_0_6(dg):
    assert dg.lib().dg_version() == b"doomgpu 0.6 (gfx950; ABI 4)"
