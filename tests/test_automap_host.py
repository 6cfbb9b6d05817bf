"""CPU tier of the 2-D map view (the reference's viewing_map frame): dg_map_lines against the numpy restatement (np_automap), line for
line, and the closed-form line steps of csrc/map_core.h against the literal SDL loop (tests/map_lines/line_check.cpp)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import np_automap as na
from test_hand_wad import build_hand_iwad, build_polygon_iwad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 40), (41, 57), (320, 200), (1024, 768), (1280, 800), (2560, 1600)]
ANGLES = [0.0, math.pi, -math.pi, math.pi / 2, 1e4, -0.0]


def _doom2_scale(synth):
    return synth.build_synth_iwad(2002, heavy=True, vanilla=True, grid=(32, 24), n_things=500)


def _flag_patched(synth):
    wad = synth.build_synth_iwad(1993)
    n = na.read_map(wad)[1]
    return na.patch_linedef_flags(wad, "E1M1", [(k, 128) for k in range(0, len(n), 3)] + [(k, 4) for k in range(1, len(n), 5)])


MAPS = {
    "synth1993": lambda s: s.build_synth_iwad(1993),
    "synth1994_heavy": lambda s: s.build_synth_iwad(1994, heavy=True),
    "synth1995_vanilla": lambda s: s.build_synth_iwad(1995, vanilla=True),
    "quirks": lambda s: s.build_synth_iwad(1993, quirks=True),
    "hand": lambda s: build_hand_iwad(),
    "polygon1200": lambda s: build_polygon_iwad(),
    "doom2_scale": _doom2_scale,
    "flags_patched": _flag_patched,
}


def views_for(mv, path):
    """(dg_view, restatement view) pairs: path records, views off the map (the arrow leaves the frame), special angles (trig_valid = 0)."""
    import importlib
    dg = importlib.import_module("doom-rust-renderer_amd")
    out = []
    for i in (0, 97, 323, 500, 728, 999):
        out.append((dg.make_views(path[i:i + 1])[0], na.path_view(path[i])))
    cx, cy = float((mv.left + mv.right) / 2), float((mv.top + mv.bottom) / 2)
    span = float(max(mv.right - mv.left, mv.bottom - mv.top, 1))
    for (x, y, a) in ((float(mv.left) - 0.3 * span, cy, 1.0), (cx, float(mv.bottom) + 0.5 * span, -2.0), (float(mv.right) + 0.01, float(mv.top) - 0.01, 0.5)):
        out.append((dg.DgView(x, y, a, 0, 0, 0, 0, 0, 0, 0), na.libm_view(x, y, a)))
    for a in ANGLES:
        out.append((dg.DgView(cx, cy, a, 0, 0, 0, 0, 0, 0, 0), na.libm_view(cx, cy, a)))
    return out


@pytest.fixture(scope="module")
def maps(synth):
    return {k: f(synth) for k, f in MAPS.items()}


@pytest.mark.parametrize("name", list(MAPS))
def test_map_lines_equal_restatement(dg, maps, path1993, name):
    wad = maps[name]
    sc = dg.Scene(wad, "E1M1")
    mv = na.MapView(wad)
    views = views_for(mv, path1993)
    for W, H in SIZES:
        base = mv.lines_for(W, H)
        got = sc.map_lines(W, H)
        assert np.array_equal(got, np.asarray(base, dtype=np.int64).reshape(-1, 5)), (name, W, H)
        for v, rv in views:
            want = np.asarray(base + mv.arrow(W, H, *rv), dtype=np.int64)
            got = sc.map_lines(W, H, v)
            assert np.array_equal(got, want), (name, W, H, rv)
    sc.close()


def test_flags_select_colour_and_dontdraw(dg, maps):
    wad = maps["flags_patched"]
    lines = na.read_map(wad)[1]
    sc = dg.Scene(wad, "E1M1")
    got = sc.map_lines(320, 200)
    drawn = [fl for _, _, fl in lines if not fl & 128]
    assert len(got) == len(drawn) < len(lines)
    assert list(got[:, 4]) == [na.YELLOW if fl & 4 else na.RED for fl in drawn]
    assert (got[:, 4] == na.YELLOW).any() and (got[:, 4] == na.RED).any()


def test_zero_extent_map_is_in_contract(dg, synth):
    """Every vertex on one x: xs = 0, every linedef point's X is NaN -> 0 (as i32)."""
    wad = synth.build_synth_iwad(1993)
    d = synth.wad_directory(wad)
    i = next(k for k, (n, _, _) in enumerate(d) if n == "E1M1")
    _, vo, vs = d[i + 4]
    b = bytearray(wad)
    for o in range(vo, vo + vs - vs % 4, 4):
        struct.pack_into("<h", b, o, 512)
    wad = bytes(b)
    sc = dg.Scene(wad, "E1M1")
    mv = na.MapView(wad)
    got = sc.map_lines(320, 200)
    assert np.array_equal(got, np.asarray(mv.lines_for(320, 200), dtype=np.int64))
    assert len(got) and (got[:, 0] == 0).all() and (got[:, 2] == 0).all()
    # an arrow whose x moves at all lands at +-inf there: out of contract on both sides
    with pytest.raises(na.OutOfContract):
        mv.lines_for(320, 200, na.libm_view(512.0, 100.0, 0.3))
    assert dg.lib().dg_map_lines(sc._h, 320, 200, dg.DgView(512.0, 100.0, 0.3, 0, 0, 0, 0, 0, 0, 0), None, 0) == dg.DG_ERR_INVALID


def test_map_lines_count_only_and_small_cap(dg, synth):
    sc = dg.Scene(synth.build_synth_iwad(1993), "E1M1")
    L = dg.lib()
    v = dg.DgView(1000.0, 1000.0, 0.5, 0, 0, 0, 0, 0, 0, 0)
    n = L.dg_map_lines(sc._h, 320, 200, v, None, 0)
    assert n == len(sc.map_lines(320, 200)) + 3
    arr = (dg.DgMapLine * n)()
    arr[0].x0 = 12345
    assert L.dg_map_lines(sc._h, 320, 200, v, arr, n - 1) == n and arr[0].x0 == 12345     # cap too small: count only
    assert L.dg_map_lines(sc._h, 320, 200, None, None, 0) == n - 3


@pytest.mark.parametrize("W,H", [(39, 40), (40, 39), (0, 0), (-5, 200), (320, 1)])
def test_map_lines_rejects_small_frames(dg, synth, W, H):
    sc = dg.Scene(synth.build_synth_iwad(1993), "E1M1")
    assert dg.lib().dg_map_lines(sc._h, W, H, None, None, 0) == dg.DG_ERR_INVALID
    with pytest.raises(dg.DoomGpuError):
        sc.map_lines(W, H, dg.DgView(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))


def test_arrow_beyond_2_pow_24_is_invalid_exactly_where_the_restatement_says(dg, synth):
    wad = synth.build_synth_iwad(1993)
    sc = dg.Scene(wad, "E1M1")
    mv = na.MapView(wad)
    W, H = 1280, 800
    scale = float(mv.right - mv.left) / (W - 40)          # map units per pixel
    seen = set()
    for k in np.linspace(0.999, 1.001, 41):
        for sign in (-1, 1):
            x = float(mv.left) + sign * k * scale * (1 << 24)
            for (px, py) in ((x, 0.0), (0.0, float(mv.top) + sign * k * scale * (1 << 24) * (H - 40) / (W - 40) * float(mv.bottom - mv.top) / float(mv.right - mv.left))):
                v = dg.DgView(px, py, 0.25, 0, 0, 0, 0, 0, 0, 0)
                try:
                    want = mv.lines_for(W, H, na.libm_view(px, py, 0.25))
                except na.OutOfContract:
                    want = None
                rc = dg.lib().dg_map_lines(sc._h, W, H, v, None, 0)
                if want is None:
                    assert rc == dg.DG_ERR_INVALID
                else:
                    assert np.array_equal(sc.map_lines(W, H, v), np.asarray(want, dtype=np.int64))
                seen.add(want is None)
    assert seen == {True, False}
    for far in (1e9, -1e9, float("inf")):
        assert dg.lib().dg_map_lines(sc._h, W, H, dg.DgView(far, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0), None, 0) == dg.DG_ERR_INVALID


@pytest.fixture(scope="module")
def line_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("map_lines") / "line_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "map_lines", "line_check.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("mode", ["exhaustive", "far", "random"])
def test_closed_form_line_steps_equal_sdl_loop(line_check, mode):
    r = subprocess.run([line_check, mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_restatement_loop_matches_vectorised_raster():
    """np_automap's vectorised raster is the literal loop run for all lines at once: check it against the scalar loop."""
    rng = np.random.default_rng(7)
    lines = [(int(a), int(b), int(c), int(d), int(rng.integers(1, 1 << 24))) for a, b, c, d in rng.integers(-30, 90, size=(300, 4))]
    img = na.rasterise(lines, 64, 48)
    ref = np.zeros((48, 64, 3), np.uint8)
    for x0, y0, x1, y1, rgb in lines:
        for x, y in na.sdl_line_points(x0, y0, x1, y1):
            if 0 <= x < 64 and 0 <= y < 48:
                ref[y, x] = (rgb & 255, (rgb >> 8) & 255, rgb >> 16)
    assert np.array_equal(img, ref)
