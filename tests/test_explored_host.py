"""CPU tier of the explored-map frames: the host entries (dg_seen_words, dg_seen_lines_host, dg_seen_accumulate_host,
dg_explored_map_host) against the numpy restatement (np_explored), and tests/explored/explored_host_main.cpp — the same entries and the
cover / chain structure the GPU draws from, as a stand-alone program under AddressSanitizer + UBSan.

  seen rows      label planes of path views of the light, heavy and vanilla-shaped maps at 160x100, 131x67 and 44x41; synthetic planes
  accumulation   run_len 1, n and a proper divisor, with and without carry_in, words 1 and 17, n = 1, the sums the contract names
  frames         all ones == dg_map_lines rasterised, all zero == black + arrow, one line, every subset of the lines meeting at a vertex,
                 a DONTDRAW line with its bit set
  errors         every error return
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import explored_cases as xc
import np_automap as na
import np_explored as ne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(160, 100), (131, 67), (44, 41)]
MAPS = {"light": ("wad1993", "path1993"), "heavy": ("wad1994", "path1994"), "vanilla": ("wad1995", "path1995")}
PATH_IDX = [0, 297, 623, 900]


@pytest.fixture(scope="module")
def worlds(dg, request):
    """Per map: the scene, the restatement, path records and per size the label planes of PATH_IDX on the CPU."""
    out = {}
    for name, (wad_fx, path_fx) in MAPS.items():
        wad, path = request.getfixturevalue(wad_fx), request.getfixturevalue(path_fx)
        sc = dg.Scene(wad, "e1m1")
        planes = {(W, H): xc.path_label_planes(dg, sc, W, H, dg.make_views(path[PATH_IDX])) for W, H in SIZES}
        out[name] = (sc, ne.Explored(wad), path, planes)
    yield out
    for sc, _, _, _ in out.values():
        sc.close()


@pytest.mark.parametrize("name", list(MAPS))
def test_seen_rows_of_path_views_equal_the_model(dg, worlds, name):
    sc, ex, _, planes = worlds[name]
    assert dg.seen_words(sc) == ex.words == (ex.n_lines + 31) // 32
    some = False
    for size, (ids, cls) in planes.items():
        got = dg.seen_lines_host(sc, ids, cls)
        want = ex.seen(ids, cls)
        assert np.array_equal(got, want), (name, size)
        some |= bool(want.any())
    assert some                                                            # the views show walls


@pytest.mark.parametrize("size", [(64, 40), (131, 67), (5, 9), (96, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_seen_rows_of_synthetic_planes(dg, worlds, size):
    sc, ex, _, _ = worlds["light"]
    W, H = size
    names, ids, cls = xc.stacked(xc.synthetic_planes(ex, W, H))
    got = dg.seen_lines_host(sc, ids, cls)
    assert np.array_equal(got, ex.seen(ids, cls))
    row = dict(zip(names, got))
    S = len(ex.seg_line)
    assert ex.n_lines % 32 != 0 and not (got[:, -1] >> np.uint32(ex.n_lines % 32)).any()          # the bits at and above L stay 0
    assert not row["other_classes_with_seg_ids"].any()
    assert ex.row_to_lines(row["ids_beyond_the_seg_count"]) == [int(ex.seg_line[5])]
    a, b, line = xc.two_sided_segs(ex)
    assert ex.row_to_lines(row["two_segs_of_one_line"]) == [line]
    assert ex.row_to_lines(row["bits_31_32_and_last"]) == sorted({int(ex.seg_line[k]) for k in (31, 32, S - 1)})
    if W * H >= S:
        assert ex.row_to_lines(row["every_pixel_another_seg"]) == sorted(set(ex.seg_line.tolist()))
    # a batch keeps its rows apart: each frame alone gives the same row
    for k in (0, len(names) - 1):
        assert np.array_equal(dg.seen_lines_host(sc, ids[k:k + 1], cls[k:k + 1])[0], got[k])


@pytest.mark.parametrize("words", [1, 17])
def test_accumulation(dg, words):
    rng = np.random.default_rng(words)
    n = 12
    seen = (rng.integers(0, 1 << 32, (n, words), dtype=np.uint64) & rng.integers(0, 1 << 32, (n, words), dtype=np.uint64)
            & rng.integers(0, 1 << 32, (n, words), dtype=np.uint64)).astype(np.uint32)
    for run_len in (1, 4, n):
        runs = n // run_len
        for carry in (None, rng.integers(0, 1 << 32, (runs, words), dtype=np.uint64).astype(np.uint32) & np.uint32(0x0F0F00FF)):
            got = dg.seen_accumulate_host(seen, run_len, carry)
            want = ne.accumulate(seen, run_len, carry)
            for k in dg.SEEN_OUTPUTS:
                assert np.array_equal(got[k], want[k]), (run_len, carry is not None, k)
            cin = np.zeros((runs, words), np.uint32) if carry is None else carry
            assert np.array_equal(got["fresh"].reshape(runs, run_len).sum(axis=1), ne.popcount(got["carry_out"] & ~cin))
            assert (np.diff(got["total"].reshape(runs, run_len).astype(np.int64), axis=1) >= 0).all()
            assert np.array_equal(got["carry_out"], got["upto"].reshape(runs, run_len, words)[:, -1])
            # any output may be left out
            for k in dg.SEEN_OUTPUTS:
                only = dg.seen_accumulate_host(seen, run_len, carry, want=(k,))
                assert list(only) == [k] and np.array_equal(only[k], want[k])
    one = dg.seen_accumulate_host(seen[:1], 1)
    assert np.array_equal(one["upto"], seen[:1]) and one["fresh"][0] == one["total"][0] == ne.popcount(seen[:1])[0]


def _views(dg, path):
    recs = path[[500]]
    return list(zip(dg.make_views(recs), [na.path_view(r) for r in recs])) + [(None, None)]


@pytest.mark.parametrize("name", list(MAPS))
def test_frames_equal_the_model(dg, worlds, name):
    sc, ex, path, planes = worlds[name]
    for W, H in SIZES:
        seen = dg.seen_lines_host(sc, *planes[(W, H)])
        masks = xc.frame_masks(ex, extra_rows=[seen[0], np.bitwise_or.reduce(seen, axis=0)])
        full = na.rasterise(ex.mv.lines_for(W, H), W, H)
        for v, rv in _views(dg, path):
            for mname, row in masks.items():
                got = dg.explored_map_host(sc, W, H, v, row)
                want = ex.frame(W, H, rv, row)
                assert np.array_equal(got, want), (name, W, H, mname, int((got != want).any(axis=2).sum()))
            if v is None:
                assert np.array_equal(dg.explored_map_host(sc, W, H, None, masks["all_ones"]), full)
                assert not dg.explored_map_host(sc, W, H, None, masks["all_zero"]).any()
            else:
                lines = sc.map_lines(W, H, v)
                assert np.array_equal(dg.explored_map_host(sc, W, H, v, masks["all_ones"]), na.rasterise([tuple(r) for r in lines.tolist()], W, H))
                assert np.array_equal(dg.explored_map_host(sc, W, H, v, masks["all_zero"]), na.rasterise(ex.mv.arrow(W, H, *rv), W, H))


def test_the_vertex_subsets_hide_the_top_line_and_show_a_lower_one(dg, worlds):
    """At the vertex pixel every subset shows the colour of the latest line of the subset; without the latest, an earlier one."""
    sc, ex, _, _ = worlds["light"]
    W, H = 160, 100
    meet = xc.meeting_lines(ex)
    assert len(meet) >= 3
    ends = [set(ex.mv.lines[l][:2]) for l in meet]
    v = set.intersection(*ends).pop()
    x, y = ex.mv.point(W, H, *ex.mv.verts[v])
    colour = lambda l: [255, 255, 0] if ex.mv.lines[l][2] & 4 else [255, 0, 0]
    for r in range(1, len(meet) + 1):
        for sub in itertools.combinations(meet, r):
            got = dg.explored_map_host(sc, W, H, None, ex.bits_to_row(sub))
            assert got[y, x].tolist() == colour(max(sub)), sub
    assert not dg.explored_map_host(sc, W, H, None, ex.bits_to_row([]))[y, x].any()


def test_a_dontdraw_line_with_its_bit_set_stays_undrawn(dg, wad1993):
    ex0 = ne.Explored(wad1993)
    hidden = [3, ex0.n_lines // 2]
    wad = na.patch_linedef_flags(wad1993, "E1M1", [(k, 128) for k in hidden])
    sc, ex = dg.Scene(wad, "e1m1"), ne.Explored(wad)
    W, H = 160, 100
    ones = ex.bits_to_row(range(ex.n_lines))
    got = dg.explored_map_host(sc, W, H, None, ones)
    assert np.array_equal(got, ex.frame(W, H, None, ones)) and np.array_equal(got, na.rasterise(ex.mv.lines_for(W, H), W, H))
    assert not np.array_equal(got, ne.Explored(wad1993).frame(W, H, None, ones))         # the two lines are missing
    assert not dg.explored_map_host(sc, W, H, None, ex.bits_to_row(hidden)).any()          # alone they draw nothing
    # the line after a hidden one is still line hidden + 1 of the mask, not hidden
    nxt = dg.explored_map_host(sc, W, H, None, ex.bits_to_row([hidden[0] + 1]))
    assert nxt.any() and np.array_equal(nxt, ex.frame(W, H, None, ex.bits_to_row([hidden[0] + 1])))
    # a seg of a hidden line still marks it seen
    seg = int(np.nonzero(ex.seg_line == hidden[0])[0][0])
    ids, cls = np.full((1, 4, 4), seg, np.uint16), np.full((1, 4, 4), 1, np.uint8)
    assert ex.row_to_lines(dg.seen_lines_host(sc, ids, cls)[0]) == [hidden[0]]
    sc.close()


def test_every_error_return(dg, worlds, wad1993):
    L = dg.lib()
    sc, ex, path, _ = worlds["light"]
    P = lambda a: a.ctypes.data_as(dg._P)
    ids, cls, seen = np.zeros((1, 4, 4), np.uint16), np.zeros((1, 4, 4), np.uint8), np.full((1, ex.words), 77, np.uint32)
    assert L.dg_seen_words(None) == dg.DG_ERR_INVALID
    assert L.dg_seen_lines_host(None, 4, 4, 1, P(ids), P(cls), P(seen)) == dg.DG_ERR_INVALID
    for args in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 16385, 1), (4, 4, -1)):
        assert L.dg_seen_lines_host(sc._h, *args, P(ids), P(cls), P(seen)) == dg.DG_ERR_INVALID, args
    for k in range(3):
        ptrs = [P(ids), P(cls), P(seen)]
        ptrs[k] = None
        assert L.dg_seen_lines_host(sc._h, 4, 4, 1, *ptrs) == dg.DG_ERR_INVALID
    assert (seen == 77).all()                                              # a refused call writes nothing
    assert L.dg_seen_lines_host(sc._h, 4, 4, 0, P(ids), P(cls), P(seen)) == dg.DG_OK and (seen == 77).all()
    assert L.dg_seen_lines_host(sc._h, 4, 4, 1, P(ids), P(cls), P(seen)) == dg.DG_OK and not seen.any()
    rows, out = np.zeros((4, 2), np.uint32), np.full((4, 2), 77, np.uint32)
    acc = lambda words, n, run_len, s=rows: L.dg_seen_accumulate_host(words, n, run_len, None, None if s is None else P(s), P(out), None, None, None)
    for args in ((0, 4, 1), (-1, 4, 1), (2, -1, 1), (2, 4, 0), (2, 4, -2), (2, 4, 3)):
        assert acc(*args) == dg.DG_ERR_INVALID, args
    assert acc(2, 4, 2, None) == dg.DG_ERR_INVALID and (out == 77).all()
    assert acc(2, 0, 1, None) == dg.DG_OK and (out == 77).all()
    assert acc(2, 4, 2) == dg.DG_OK and not out.any()
    assert L.dg_seen_accumulate_host(2, 4, 2, None, P(rows), None, None, None, None) == dg.DG_OK
    v = dg.make_views(path[:1])
    row, img = ex.bits_to_row([1]), np.zeros((100, 160, 3), np.uint8)
    assert L.dg_explored_map_host(None, 160, 100, v, P(row), P(img)) == dg.DG_ERR_INVALID
    assert L.dg_explored_map_host(sc._h, 160, 100, v, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_explored_map_host(sc._h, 160, 100, v, P(row), None) == dg.DG_ERR_INVALID
    for W, H in ((39, 40), (40, 39), (16385, 100)):
        assert L.dg_explored_map_host(sc._h, W, H, v, P(row), P(img)) == dg.DG_ERR_INVALID, (W, H)
    far = (dg.DgView * 1)(dg.DgView(1e12, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
    assert L.dg_explored_map_host(sc._h, 160, 100, far, P(row), P(img)) == dg.DG_ERR_INVALID      # the arrow beyond +-2^24
    assert not img.any()
    assert L.dg_explored_map_host(sc._h, 160, 100, v, P(row), P(img)) == dg.DG_OK and img.any()
    # a scene past the limit of label frames (65 537 segs): DG_ERR_CAPACITY, nothing written; 65 537 linedefs are no limit of the host entries
    big = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 5, 12, 65537), "e1m1")
    seen[:] = 77
    assert L.dg_seen_lines_host(big._h, 4, 4, 1, P(ids), P(cls), P(seen)) == dg.DG_ERR_CAPACITY and (seen == 77).all()
    big.close()
    many = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 2, 14, 65537), "e1m1")
    assert dg.seen_words(many) == 2049
    wide = np.full((1, 2049), 77, np.uint32)
    assert L.dg_seen_lines_host(many._h, 4, 4, 1, P(ids), P(cls), P(wide)) == dg.DG_OK and not wide.any()
    assert L.dg_explored_map_host(many._h, 160, 100, v, P(wide), P(img)) == dg.DG_OK
    many.close()
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    assert L.dg_seen_lines_device(None, 4, 4, 1, P(ids), P(cls), P(seen)) == dg.DG_ERR_INVALID
    assert L.dg_slot_seen_lines(None, 0, 0, 1, 1, None, None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_ctx_seen_kernel_ms(None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_submit_explored_map_views(None, 0, v, 1, P(row)) == dg.DG_ERR_INVALID
    assert L.dg_render_explored_map_views(None, v, 1, P(row), None) == dg.DG_ERR_INVALID


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_seen_words", "dg_seen_lines_host", "dg_seen_accumulate_host", "dg_explored_map_host", "dg_seen_lines_device", "dg_slot_seen_lines",
             "dg_ctx_seen_kernel_ms", "dg_submit_explored_map_views", "dg_render_explored_map_views"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert dg.DG_FE_MAP_EXPLORED == 8 and b"ABI 4" in dg.lib().dg_version()


def test_the_host_entries_and_the_cover_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/explored/explored_host_main.cpp (its own main) with the host sources of the library, built with -fsanitize=address,undefined
    and run as a program: the three host entries, and the cover / chain builder plus explored_pick against the literal rule pixel for
    pixel.  It checks its own results, and any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "explored_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "explored", "explored_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "light.wad"
    wad.write_bytes(wad1993)
    r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "explored_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
