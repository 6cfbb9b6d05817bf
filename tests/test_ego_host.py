"""CPU tier of the player-centred map frames: dg_ego_map_lines and dg_ego_map_host against the numpy restatement (np_ego), and
tests/ego/ego_host_main.cpp — the same entries, the band property and the kernel's three phases as a host loop — as a stand-alone
program under AddressSanitizer + UBSan.

  maps     the light map, the heavy map, the hand-assembled WAD
  sizes    64x40, 44x41, 131x67, 320x200
  scales   2^-10, 0.05 (the whole level in the frame), 1, 8, 64 (a few lines crossing the whole frame from endpoints far outside it)
  views    headings 0, pi/2, pi with trig_valid = 0, path views with trig_valid = 1, a view far outside the level, a view on a vertex
  masks    NULL == all ones, all zero == black + arrow, one line, every subset of three lines meeting at a vertex, a DONTDRAW line
  errors   every error return
"""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import explored_cases as xc
import np_automap as na
import np_ego as ng
from test_hand_wad import build_hand_iwad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 40), (44, 41), (131, 67), (320, 200)]
SCALES = [2.0 ** -10, 0.05, 1.0, 8.0, 64.0]
FLAGS = [0, ng.ROTATE, ng.ARROW, ng.ROTATE | ng.ARROW]
PATH_IDX = [0, 297, 623, 900]


def _view(dg, x, y, angle):
    """(dg_view with trig_valid = 0, the model's view with the libm trig the library will take)."""
    return dg.DgView(float(x), float(y), float(angle), 0, 0, 0, 0, 0, 0, 0), na.libm_view(x, y, angle)


def _views(dg, model, path):
    """[(name, dg_view, model view)]."""
    cx, cy = (float(np.float32(t)) for t in (path[500][0], path[500][1])) if path is not None else (float(model.verts[0][0]) + 13.5, float(model.verts[0][1]) - 7.25)
    out = [(f"heading_{n}", *_view(dg, cx, cy, a)) for n, a in (("0", 0.0), ("half_pi", math.pi / 2), ("pi", math.pi))]
    if path is not None:
        out += [(f"path_{i}", v, na.path_view(path[i])) for i, v in zip(PATH_IDX, dg.make_views(path[PATH_IDX]))]
    out.append(("far_outside", *_view(dg, 60000.0, -61234.5, 0.7)))
    vx, vy = model.verts[model.lines[len(model.lines) // 2][0]]
    out.append(("on_a_vertex", *_view(dg, float(vx), float(vy), 2.1)))
    return out


def _meeting_lines(model, at_least: int = 3):
    """The drawn linedefs (ascending) that share the first vertex at which at_least of them meet."""
    by_vertex = {}
    for l, (v1, v2, fl) in enumerate(model.lines):
        if not fl & 128:
            for v in {v1, v2}:
                by_vertex.setdefault(v, []).append(l)
    return next(by_vertex[v] for v in sorted(by_vertex) if len(by_vertex[v]) >= at_least)


@pytest.fixture(scope="module")
def worlds(dg, wad1993, wad1994, path1993, path1994):
    out = {}
    for name, wad, path in (("light", wad1993, path1993), ("heavy", wad1994, path1994), ("hand", build_hand_iwad(), None)):
        sc, model = dg.Scene(wad, "e1m1"), ng.EgoModel(wad)
        out[name] = (sc, model, _views(dg, model, path))
    yield out
    for sc, _, _ in out.values():
        sc.close()


def test_the_frame_entry_of_the_model_equals_the_whole_literal_loop():
    """np_ego.enter_frame (used for lines too long to run from their start) against np_automap.sdl_line_points."""
    rng = np.random.default_rng(5)
    W, H = 64, 40
    some = 0
    for i in range(1500):
        x0, y0, x1, y1 = (int(t) for t in rng.integers(-3000, 3000, 4) // (1 if i % 3 == 0 else 12))
        if rng.integers(0, 4) == 0:
            x1 = x0 + int(rng.integers(-2, 3))                              # steep and flat lines, single points
        if rng.integers(0, 4) == 0:
            y1 = y0
        whole = [(x, y) for x, y in na.sdl_line_points(x0, y0, x1, y1) if 0 <= x < W and 0 <= y < H]
        st = ng.enter_frame((x0, y0, x1, y1, 0), W, H)
        tail = [] if st is None else [(x, y) for x, y in ng.sdl_tail_points(*st) if 0 <= x < W and 0 <= y < H]
        assert tail == whole, (x0, y0, x1, y1)
        some += bool(whole)
    assert some > 50


@pytest.mark.parametrize("name", ["light", "heavy", "hand"])
def test_lines_equal_the_model(dg, worlds, name):
    sc, model, views = worlds[name]
    k = 0
    for (W, H), scale, flags in itertools.product(SIZES, SCALES, FLAGS):
        for vname, v, mv in (views[k % len(views)], views[(k + 3) % len(views)]):
            got = dg.ego_map_lines(sc, W, H, v, (scale, flags))
            want = model.lines_for(W, H, mv, scale, flags)
            assert [tuple(r) for r in got.tolist()] == want, (name, W, H, scale, flags, vname)
        k += 1


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["light", "heavy", "hand"])
def test_frames_equal_the_model(dg, worlds, name, size):
    sc, model, views = worlds[name]
    W, H = size
    ones = model.bits_to_row(range(model.n_lines))
    rng = np.random.default_rng(W)
    half = (rng.integers(0, 1 << 32, model.words, dtype=np.uint64).astype(np.uint32)) & ones
    masks = [None, ones, half, np.zeros(model.words, np.uint32), model.bits_to_row([model.n_lines // 2])]
    k = SIZES.index(size)
    lit = 0
    for scale, rotate in itertools.product(SCALES, (0, ng.ROTATE)):
        vname, v, mv = views[k % len(views)]
        flags = rotate | (ng.ARROW if k % 3 else 0)
        mask = masks[k % len(masks)]
        got = dg.ego_map_host(sc, W, H, v, (scale, flags), mask)
        want = model.frame(W, H, mv, scale, flags, mask)
        assert np.array_equal(got, want), (name, W, H, scale, flags, vname, k % len(masks), int((got != want).any(axis=2).sum()))
        lit += int(got.any())
        k += 1
    assert lit >= 4
    # every view once more at scale 1, heading up with the arrow: the far view is black + arrow
    for vname, v, mv in views:
        got = dg.ego_map_host(sc, W, H, v, (1.0, ng.ROTATE | ng.ARROW))
        assert np.array_equal(got, model.frame(W, H, mv, 1.0, ng.ROTATE | ng.ARROW)), (name, vname)
        if vname == "far_outside":
            assert np.array_equal(got, ng.rasterise(ng.arrow(W, H, mv, 1.0, True), W, H)) and got.any()
            assert not dg.ego_map_host(sc, W, H, v, (1.0, ng.ROTATE)).any()


def test_masks(dg, worlds):
    sc, model, views = worlds["light"]
    W, H = 131, 67
    _, v, mv = views[4]
    ones = model.bits_to_row(range(model.n_lines))
    for scale, flags in ((0.05, ng.ARROW), (1.0, ng.ROTATE | ng.ARROW)):
        p = (scale, flags)
        assert np.array_equal(dg.ego_map_host(sc, W, H, v, p, None), dg.ego_map_host(sc, W, H, v, p, ones))
        assert dg.ego_map_host(sc, W, H, v, p, ones).any()
        zero = dg.ego_map_host(sc, W, H, v, p, np.zeros(model.words, np.uint32))
        assert np.array_equal(zero, ng.rasterise(ng.arrow(W, H, mv, scale, bool(flags & ng.ROTATE)), W, H)) and zero.any()
        assert not dg.ego_map_host(sc, W, H, v, (scale, flags & ~ng.ARROW), np.zeros(model.words, np.uint32)).any()
        one = model.bits_to_row([model.n_lines // 2])
        assert np.array_equal(dg.ego_map_host(sc, W, H, v, p, one), model.frame(W, H, mv, scale, flags, one))


def test_the_vertex_subsets_show_the_latest_line_of_the_subset(dg, worlds):
    """The view sits on a vertex where three lines meet: the vertex is pixel (W/2, H/2), and every subset shows its latest line there."""
    sc, model, _ = worlds["light"]
    meet = _meeting_lines(model)
    assert len(meet) >= 3
    vtx = set.intersection(*[set(model.lines[l][:2]) for l in meet]).pop()
    vx, vy = model.verts[vtx]
    W, H = 64, 40
    colour = lambda l: [255, 255, 0] if model.lines[l][2] & 4 else [255, 0, 0]
    for flags in (0, ng.ROTATE):
        v, mv = _view(dg, float(vx), float(vy), 0.9)
        for r in range(1, len(meet) + 1):
            for sub in itertools.combinations(meet, r):
                row = model.bits_to_row(sub)
                got = dg.ego_map_host(sc, W, H, v, (0.25, flags), row)
                assert got[H // 2, W // 2].tolist() == colour(max(sub)), (flags, sub)
                assert np.array_equal(got, model.frame(W, H, mv, 0.25, flags, row))
        assert not dg.ego_map_host(sc, W, H, v, (0.25, flags), model.bits_to_row([]))[H // 2, W // 2].any()


def test_a_dontdraw_line_with_its_bit_set_stays_undrawn(dg, wad1993, path1993):
    m0 = ng.EgoModel(wad1993)
    hidden = [3, m0.n_lines // 2]
    wad = na.patch_linedef_flags(wad1993, "E1M1", [(k, 128) for k in hidden])
    sc, model = dg.Scene(wad, "e1m1"), ng.EgoModel(wad)
    W, H, p = 131, 67, (0.01, 0)                                                                 # the whole level in the frame
    v, mv = dg.make_views(path1993[[500]])[0], na.path_view(path1993[500])
    ones = model.bits_to_row(range(model.n_lines))
    got = dg.ego_map_host(sc, W, H, v, p, ones)
    assert np.array_equal(got, model.frame(W, H, mv, *p, ones)) and np.array_equal(got, dg.ego_map_host(sc, W, H, v, p))
    assert not np.array_equal(got, m0.frame(W, H, mv, *p, ones))                                  # the two lines are missing
    assert not dg.ego_map_host(sc, W, H, v, p, model.bits_to_row(hidden)).any()                   # alone they draw nothing
    nxt = model.bits_to_row([hidden[0] + 1])                                                       # the line after a hidden one keeps its own bit
    assert dg.ego_map_host(sc, W, H, v, p, nxt).any() and np.array_equal(dg.ego_map_host(sc, W, H, v, p, nxt), model.frame(W, H, mv, *p, nxt))
    assert len(dg.ego_map_lines(sc, W, H, v, p)) == model.n_lines - 2
    sc.close()


def test_every_error_return(dg, worlds, wad1993):
    L = dg.lib()
    sc, model, views = worlds["light"]
    P = lambda a: a.ctypes.data_as(dg._P)
    good_v = dg.DgView(100.0, 200.0, 0.5, 0, 0, 0, 0, 0, 0, 0)
    good_p = dg.DgEgoMap(1.0, 3)
    img = np.zeros((40, 64, 3), np.uint8)
    n_lines = L.dg_ego_map_lines(sc._h, 64, 40, ctypes.byref(good_v), ctypes.byref(good_p), None, 0)
    assert n_lines == sum(1 for _, _, fl in model.lines if not fl & 128) + 3

    def both(W, H, v, p):
        """The two host entries' return codes, which must agree; a refused call writes nothing."""
        img[:] = 0
        a = L.dg_ego_map_lines(sc._h, W, H, ctypes.byref(v), ctypes.byref(p), None, 0)
        b = L.dg_ego_map_host(sc._h, W, H, ctypes.byref(v), ctypes.byref(p), None, P(img))
        assert (a < 0) == (b < 0) and (a >= 0 or a == b) and (b == dg.DG_OK or not img.any())
        return b

    assert both(64, 40, good_v, good_p) == dg.DG_OK and img.any()
    big = np.zeros((16384 * 16 * 3,), np.uint8)
    for W, H in ((15, 40), (64, 15), (16385, 40), (64, 16385), (0, 40), (-1, 40)):
        assert both(W, H, good_v, good_p) == dg.DG_ERR_INVALID, (W, H)
    assert L.dg_ego_map_host(sc._h, 16, 16, ctypes.byref(good_v), ctypes.byref(good_p), None, P(big)) == dg.DG_OK
    assert L.dg_ego_map_host(sc._h, 16384, 16, ctypes.byref(good_v), ctypes.byref(good_p), None, P(big)) == dg.DG_OK
    for scale in (0.0, -1.0, 2.0 ** -11, 64.5, float("nan"), float("inf")):
        assert both(64, 40, good_v, dg.DgEgoMap(scale, 3)) == dg.DG_ERR_INVALID, scale
    for scale in (2.0 ** -10, 64.0):
        assert both(64, 40, good_v, dg.DgEgoMap(scale, 3)) == dg.DG_OK, scale
    for flags in (4, 8, 0x80000000, 7):
        assert both(64, 40, good_v, dg.DgEgoMap(1.0, flags)) == dg.DG_ERR_INVALID, flags
    for bad in (65537.0, -65537.0, float("nan"), float("inf"), -float("inf")):
        assert both(64, 40, dg.DgView(bad, 0.0, 0.5, 0, 0, 0, 0, 0, 0, 0), good_p) == dg.DG_ERR_INVALID, bad
        assert both(64, 40, dg.DgView(0.0, bad, 0.5, 0, 0, 0, 0, 0, 0, 0), good_p) == dg.DG_ERR_INVALID, bad
    assert both(64, 40, dg.DgView(65536.0, -65536.0, 0.5, 0, 0, 0, 0, 0, 0, 0), good_p) == dg.DG_OK
    for bad in (1.5, -1.5, float("nan"), float("inf")):                      # trig_valid = 1: the caller's cos_a / sin_a
        assert both(64, 40, dg.DgView(0.0, 0.0, 0.5, 0, bad, 0.0, 0, 0, 0, 1), good_p) == dg.DG_ERR_INVALID, bad
        assert both(64, 40, dg.DgView(0.0, 0.0, 0.5, 0, 0.0, bad, 0, 0, 0, 1), good_p) == dg.DG_ERR_INVALID, bad
    assert both(64, 40, dg.DgView(0.0, 0.0, 0.5, 0, 1.0, -1.0, 0, 0, 0, 1), good_p) == dg.DG_OK
    # NULL arguments
    v, p = ctypes.byref(good_v), ctypes.byref(good_p)
    assert L.dg_ego_map_lines(None, 64, 40, v, p, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_lines(sc._h, 64, 40, None, p, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_lines(sc._h, 64, 40, v, None, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_host(None, 64, 40, v, p, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_host(sc._h, 64, 40, None, p, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_host(sc._h, 64, 40, v, None, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_host(sc._h, 64, 40, v, p, None, None) == dg.DG_ERR_INVALID
    # cap too small: the count comes back and nothing is written (dg_map_lines' convention)
    arr = (dg.DgMapLine * n_lines)()
    assert L.dg_ego_map_lines(sc._h, 64, 40, v, p, arr, n_lines - 1) == n_lines and not any(bytes(arr))
    assert L.dg_ego_map_lines(sc._h, 64, 40, v, p, arr, -1) == n_lines and not any(bytes(arr))
    assert L.dg_ego_map_lines(sc._h, 64, 40, v, p, arr, n_lines) == n_lines and any(bytes(arr))
    # 65 536 linedefs: DG_ERR_CAPACITY; 65 535 are drawn
    many = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 2, 14, 65536), "e1m1")
    assert L.dg_ego_map_lines(many._h, 64, 40, v, p, None, 0) == dg.DG_ERR_CAPACITY
    img[:] = 0
    assert L.dg_ego_map_host(many._h, 64, 40, v, p, None, P(img)) == dg.DG_ERR_CAPACITY and not img.any()
    many.close()
    most = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 2, 14, 65535), "e1m1")
    assert L.dg_ego_map_host(most._h, 64, 40, v, p, None, P(img)) == dg.DG_OK
    most.close()
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    assert L.dg_submit_ego_map_views(None, 0, v, 1, p, None) == dg.DG_ERR_INVALID
    assert L.dg_render_ego_map_views(None, v, 1, p, None, None) == dg.DG_ERR_INVALID


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_ego_map_lines", "dg_ego_map_host", "dg_submit_ego_map_views", "dg_render_ego_map_views"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert dg.DG_FE_MAP_EGO == 9 and (dg.DG_EGO_ROTATE, dg.DG_EGO_ARROW) == (1, 2) and ctypes.sizeof(dg.DgEgoMap) == 8
    assert dg.lib().dg_version() == b"doomgpu 0.6 (gfx950; ABI 4)"
    assert callable(dg.ego_map_lines) and callable(dg.ego_map_host) and callable(dg.Context.submit_ego_map) and callable(dg.Context.render_ego_map)
    header = open(dg.INCLUDE).read()
    assert "DG_FE_MAP_EGO = 9" in header and "typedef struct dg_ego_map { float scale; uint32_t flags; } dg_ego_map;" in header


def test_the_host_entries_the_band_property_and_the_kernel_phases_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/ego/ego_host_main.cpp (its own main) with the host sources of the library, built with -fsanitize=address,undefined and run as
    a program: the two host entries with buffers of exactly the contract's sizes against plain loops, the band property for every band
    height, and dg_ego_tiles' phases as a host loop against dg_ego_map_host.  It checks its own results; any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "ego_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "ego", "ego_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "light.wad"
    wad.write_bytes(wad1993)
    r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "ego_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
