"""The tile rasteriser's span classes and chunk paths at their boundaries (cases: tests/raster_class_cases.py).

dg_raster_tiles picks a mapper per span (the "plain" bit of DevRSpan word 0) and a path per (column, 64-row tile) chunk.  Each condition below
has a case that sits on it, and the coverage table (COVERAGE, checked on the CPU through the observer emul_bind.EmulScene.observe_lists) keeps
a later edit of the cases from silently leaving a class or path untested.  The expected frames come from tests/np_mappers.py.
  CPU tier: oracle (dr_draw_lists) == numpy, emulator == numpy, the coverage table, the brightness facts of the light cases.
  GPU tier: dg_draw_lists == numpy, all cases of a size in one batch and in reverse order, DOOMGPU_FRAME_PER_XCD 0 and 1.

Span classes (raster_core.h)                                                         case                      guards
  wall, height not a power of two (resolve_wall_span :187 `pot`)                     walls_TALL72*, mix*       wall_offset_tile's vote kernels.hip:145
  wall, |h + ay uy1| < 32000 on the first row (:193,195), both signs, d = +-1         walls_* groups first_out  wall_offset_plain kernels.hip:183-200
  wall, the same on the last row (:194,195)                                          walls_* groups last_out   (bare v_cvt_i32_f32, no `as i16`)
  wall, rows crossing +32767 / -32768, offset_y 0 / 30000 / -32768                   walls_* columns 48..59    f32_as_i16 + wrapping add, kernels.hip:143-146
  wall, d == 0 (:186,192: uy1 := NaN)                                                walls_* columns 60..63    div_prepared_nofix with d == 0, kernels.hip:142
  the same as possibly-transparent spans (has_holes -> immediate)                    walls_HOLEY1/GRATE1/COMBO2  span_texel<false> in overlay_loop, kernels.hip:311-329
  flat, lightf < 7 (resolve_flat_span :214): 1784 | 1785                             lights_wz+-2000           flat_offset_plain's missing upper clamp, kernels.hip:222-224
  flat, light 2041 | 2042, -32768, 32767; wx beyond +-32767                          lights_wz+-2000           light factor at saturated distance
  flat, div_guard_ok(gwz), div_guard_ok(wz vx) (:110-113,214): 2^64, 2^65, 2^70      guard_below/at_2^64/65, guard_wide_out   the votes of flat_offset_tile kernels.hip:168
  flat, GCFX wz = +-inf / NaN (floor_height 3e38, inf, NaN), wz == 0 exactly          guard_3e38 .. guard_wz_zero              plain divides, kernels.hip:172-173
  (div_guard_ok tests the exponent: the band is 2^-64 <= |n| < 2^65, so 2^64 itself is inside; the cases straddle both 2^64 and 2^65.
   The lower edge cannot be reached through dg_draw_lists: raster_class_cases docstring.)
Chunk paths (kernels.hip strip_body; restated once in tests/emul/emul.cpp classify_strip_paths)
  SOLE_WALL  ucol_wall :529, stage1 :566-572                                         walls_BRICK1 tile rows 0, 1; overlays
  SOLE_FLAT  ucol_flat :530, off in the tile that holds vy == 0                      lights / guard tile row 0 (72x136), rows 0..2 (72x137)
  WALK       owner_loop :578 + owner_texel :335-355 (<= 8 spans)                     plain flat in the horizon tile: lights 72x136 tile row 1; mix
  BIG        big_column_owner :370-381, :574-576 (> 8 spans)                         *_piled, the piled columns of lights / guard / overlays
  PACKED     few_rows && nk == WAVES && walk2 == 0 :537-558                          72x136 tile row 2 of every unpiled case; mix: one class per column of a wave
  overlays   overlay_loop :311 / big_column_overlays :383, `under` :533              overlays (before / after on each path; after, in the 8-row tile)
  The 8-column strip (columns 64..71) runs with nk == WAVES like any other — its waves find seven empty columns — so it does take the
  packed pass; nk != WAVES needs more than SPAN_CAP spans in a strip (test_raster_shapes.py covers that staging).
  72x137 has 9 live rows in its last tile row (never packed) and no vy == 0 row (ucol_flat stays on; |vy| = 0.5 next to the horizon).

The reference refuses none of the cases.
"""
import time

import numpy as np
import pytest

import emul_bind
import np_mappers as nm
import raster_class_cases as rc
from emul_bind import OV_HIT, OV_UNDER, OV_WALK, PATH_MASK, PATHS, PF_BEFORE, PF_HOLE, PF_SHOWS, REASONS
from test_edge_kats import to_dg_lists, view_dict

SIZES = rc.SIZES
IDS = [f"{w}x{h}" for w, h in SIZES]
PATH_NAME = {v: k for k, v in PATHS.items()}
WALL_REASONS = ["npot", "d0", "first_out", "last_out"]
FLAT_REASONS = ["gwz_out", "wzvx_out", "light7"]
# (path, class of the owning span) -> at least 8 pixels (one packed-pass column) somewhere in the case set
COVERAGE = [(p, "plain_wall") for p in ("SOLE_WALL", "WALK", "BIG", "PACKED")] + \
           [(p, "plain_flat") for p in ("SOLE_FLAT", "WALK@horizon", "BIG", "PACKED")] + \
           [(p, r) for p in ("WALK", "BIG", "PACKED") for r in WALL_REASONS + FLAT_REASONS]


@pytest.fixture(scope="module")
def np_wad(wad1993):
    return nm.Wad(wad1993)


_EXPECTED, _OBSERVED = {}, {}


def expected_frames(campath_mod, np_wad, size):
    """[(name, rec, lists, notes, numpy frame)] of a size, computed once for both tiers."""
    if size not in _EXPECTED:
        out = []
        for name, view, lists, notes in rc.CASES[size]:
            rec, vd = view_dict(campath_mod, *view)
            out.append((name, rec, lists, notes, nm.draw_lists(np_wad, "SKY1", size[0], size[1], vd, lists)))
        _EXPECTED[size] = out
    return _EXPECTED[size]


@pytest.fixture(scope="module")
def host(dg, wad1993):
    """The product's scene on the host (texture and flat ids for the lists) and the emulator's."""
    return dg.Scene(wad1993, "e1m1"), emul_bind.EmulScene(wad1993)


def observed(dg, host, campath_mod, size):
    """[(name, lists, notes, view floor_height, observer dict)] of a size."""
    if size not in _OBSERVED:
        scene, emul = host
        out = []
        for name, view, lists, notes in rc.CASES[size]:
            fl, keep = to_dg_lists(dg, scene, view_dict(campath_mod, *view)[0], lists)
            out.append((name, lists, notes, view[3], emul.observe_lists(size[0], size[1], fl)))
        _OBSERVED[size] = out
    return _OBSERVED[size]


def reason_names(mask):
    return {n for n, b in REASONS.items() if mask & b}


def span_sources(lists):
    """rec of a span (the observer's column 7) -> index of its render record / visplane: the n-th command of its kind in the order list."""
    walls = [i for k, i in lists["order"] if k == 0]
    planes = [i for k, i in lists["order"] if k == 1 and "SKY" not in lists["visplanes"][i]["flat"]]
    return walls, planes


def span_classes(span):
    """The classes of the coverage table one observed span counts for."""
    x, ctop, cbot, kind, plain, imm, reason, rec = (int(t) for t in span)
    if kind == 2:
        return {"sky"}
    if plain:
        return {"plain_wall" if kind == 0 else "plain_flat"}
    return reason_names(reason)


def pixel_paths(obs, W, H):
    return (obs["chunks"][(np.arange(H) // 64)[:, None], np.arange(W)[None, :]] & PATH_MASK)


def _diff(got, want, label):
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert len(bad) == 0, f"{label}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------

def test_the_bitmap_heights_the_cases_assume(np_wad):
    for name, h in rc.TEX_H.items():
        assert np_wad.texture(name)[1] == h, name
    for name in rc.HOLEY:
        assert any(t is None for row in np_wad.texture(name)[2] for t in row), name


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_oracle_equals_independent_restatement(oracle_scene1993, campath_mod, np_wad, size):
    W, H = size
    for name, rec, lists, notes, want in expected_frames(campath_mod, np_wad, size):
        got = np.frombuffer(oracle_scene1993.draw_lists(W, H, rec, lists), dtype=np.uint8).reshape(H, W, 3)
        _diff(got, want, name)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_emulator_equals_independent_restatement(dg, host, campath_mod, np_wad, size):
    W, H = size
    scene, emul = host
    for name, rec, lists, notes, want in expected_frames(campath_mod, np_wad, size):
        fl, keep = to_dg_lists(dg, scene, rec, lists)
        got = np.frombuffer(emul.draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)
        _diff(got, want, name)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_every_span_has_the_class_its_float32_restatement_gives(dg, host, campath_mod, size):
    """The plain bit and the reason the observer reads next to resolve_*_span equal raster_class_cases.wall_reasons / flat_reasons, which
    restate the class conditions in numpy.float32 from the list records."""
    W, H = size
    for name, lists, notes, floor_height, obs in observed(dg, host, campath_mod, size):
        walls, planes = span_sources(lists)
        for span in obs["spans"]:
            x, ctop, cbot, kind, plain, imm, reason, rec = (int(t) for t in span)
            if kind == 0:
                r = lists["renders"][walls[rec]]
                col = next(c for c in lists["columns"][r["first_column"]: r["first_column"] + r["n_columns"]]
                           if c[0] == x and max(c[1], 0) == ctop and min(c[2], H - 1) == cbot)
                want = rc.wall_reasons(rc.TEX_H[r["texture"]], ctop, cbot, col[4], col[3], np.float32(r["top_height"]) - np.float32(r["bottom_height"]))
                assert imm == (r["texture"] in rc.HOLEY)
            elif kind == 1:
                p = lists["visplanes"][planes[rec]]
                want = rc.flat_reasons(W, H, x, p["height"], floor_height, p["light_level"])
            else:
                continue
            assert reason_names(reason) == want and bool(plain) == (not want), (name, span.tolist(), want)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_each_boundary_group_has_both_sides(dg, host, campath_mod, size):
    """Of the float32 neighbours of one boundary value, some are plain and the others carry exactly the intended reason."""
    groups = 0
    for name, lists, notes, floor_height, obs in observed(dg, host, campath_mod, size):
        walls, planes = span_sources(lists)
        by_render = {}
        for span in obs["spans"]:
            if int(span[3]) == 0:
                by_render.setdefault(walls[int(span[7])], set()).add(frozenset(reason_names(int(span[6])) - {"npot"}))
        for label, intent, renders in notes["groups"]:
            seen = set().union(*[by_render[r] for r in renders])
            assert seen == {frozenset(), frozenset({intent})}, (name, label, seen)
            groups += 1
    assert groups >= 16


def test_the_guard_cases_sit_on_both_sides_of_the_band(dg, host, campath_mod):
    size = SIZES[0]
    by_name = {name: obs for name, lists, notes, fh, obs in observed(dg, host, campath_mod, size)}
    flat = lambda name: [reason_names(int(s[6])) for s in by_name[name]["spans"] if int(s[3]) == 1]
    for inside in ("guard_below_2^64", "guard_at_2^64", "guard_below_2^65", "guard_wz_zero"):
        assert all(not r for r in flat(inside)), inside
    for outside in ("guard_at_2^65", "guard_neg_at_2^65", "guard_3e38", "guard_neg_3e38", "guard_inf", "guard_neg_inf", "guard_nan"):
        assert all("gwz_out" in r for r in flat(outside)), outside
    assert any("wzvx_out" in r for r in flat("guard_at_2^65")) and any("wzvx_out" not in r for r in flat("guard_at_2^65"))     # column 0 | the rest
    n = sum("wzvx_out" in r for r in flat("guard_wide_out"))
    assert n > len(flat("guard_wide_out")) // 2 and n < len(flat("guard_wide_out"))                                               # vx == 0 in column 36
    assert all("wzvx_out" in r for r in flat("guard_inf"))                                                                      # inf * 0 = NaN there


def test_coverage_table(dg, host, campath_mod):
    """Every (path, owner class) of COVERAGE owns at least 8 pixels somewhere in the case set."""
    count = {}
    for size in SIZES:
        W, H = size
        for name, lists, notes, floor_height, obs in observed(dg, host, campath_mod, size):
            own, path = obs["owner"], pixel_paths(obs, W, H)
            horizon_tile = (H // 2) // 64 if H % 2 == 0 else -1
            tile = np.broadcast_to((np.arange(H) // 64)[:, None], (H, W))
            m = own >= 0
            keys, n = np.unique(np.stack([own[m], path[m], tile[m]]), axis=1, return_counts=True)
            for (o, p, t), c in zip(keys.T, n):
                for cls in span_classes(obs["spans"][o]):
                    count[(PATH_NAME[int(p)], cls)] = count.get((PATH_NAME[int(p)], cls), 0) + int(c)
                    if t == horizon_tile:
                        count[(PATH_NAME[int(p)] + "@horizon", cls)] = count.get((PATH_NAME[int(p)] + "@horizon", cls), 0) + int(c)
    missing = [(k, count.get(k, 0)) for k in COVERAGE if count.get(k, 0) < 8]
    assert not missing, missing


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_each_mix_chunk_holds_all_of_its_owner_classes(dg, host, campath_mod, size):
    W, H = size
    checked = set()
    for name, lists, notes, floor_height, obs in observed(dg, host, campath_mod, size):
        path = pixel_paths(obs, W, H)
        for want_path, t, cols in notes["mixes"]:
            (r0, r1) = rc.tile_rows(H)[t]
            classes = set()
            for x in cols:
                for y in range(r0, r1 + 1):
                    o = obs["owner"][y, x]
                    classes |= {"none"} if o < 0 else span_classes(obs["spans"][o])
                    assert o < 0 or PATH_NAME[int(path[y, x])] == want_path, (name, want_path, x, y, PATH_NAME[int(path[y, x])])
            assert classes >= rc.MIX_CLASSES, (name, want_path, t, cols, classes)
            checked.add(want_path)
    assert checked == ({"WALK", "BIG", "PACKED"} if H - 128 <= 8 else {"WALK", "BIG"})


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_each_overlay_placement_is_found_as_built(dg, host, campath_mod, size):
    W, H = size
    seen = set()
    for name, lists, notes, floor_height, obs in observed(dg, host, campath_mod, size):
        for want_path, t, cols, where in notes["overlays"]:
            (r0, r1) = rc.tile_rows(H)[t]
            chunks, pf = obs["chunks"][t, cols], obs["pflags"][r0:r1 + 1, cols]
            assert all(PATH_NAME[int(c) & PATH_MASK] == want_path for c in chunks), (name, want_path, where, chunks)
            if where == "after":
                assert all(c & OV_WALK and c & OV_HIT and not c & OV_UNDER for c in chunks)
                assert (pf & PF_SHOWS).astype(bool).sum() >= 8 and not (pf & PF_BEFORE).any()
                assert t != 0 or (pf & PF_HOLE).astype(bool).sum() >= 8                           # (the tall spans of tile row 0 meet holes too)
            else:
                assert (pf & PF_BEFORE).astype(bool).sum() >= 8 and not (pf & (PF_SHOWS | PF_HOLE)).any()
                if want_path.startswith("SOLE"):
                    assert all(c & OV_UNDER and not c & (OV_WALK | OV_HIT) for c in chunks)          # dropped by the pre-filter
                else:
                    assert all(c & OV_WALK and c & OV_HIT and not c & OV_UNDER for c in chunks)      # walked, loses against `winner`
            seen.add((want_path, t, where))
    assert seen == {(p, 0, w) for p in ("SOLE_WALL", "SOLE_FLAT", "WALK", "BIG") for w in ("after", "before")} | {("SOLE_WALL", 2, "after")}
    # the holey span drawn BEFORE a sole owner in the 8-row tile does not keep it off the packed pass (mix, class 4 columns)
    if H - 128 <= 8:
        mix = next(obs for name, lists, notes, fh, obs in observed(dg, host, campath_mod, size) if name == "mix")
        assert all(int(c) == PATHS["PACKED"] | OV_UNDER for c in mix["chunks"][2, 32:40])


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_light_levels_at_saturated_distance(campath_mod, np_wad, size):
    """From the numpy frames alone: where `wx as i16` is 32767, the planes lit 2042 and brighter have pixels that are not black and the planes
    lit 1784 (the brightest plain ones) have none — a kernel that took the short form for 1785 and up could not pass by luck.  Where wx is
    <= -32768 every plane but the one lit -32768 is visible."""
    W, H = size
    k = rc.frame_consts(W, H)
    for name, rec, lists, notes, want in expected_frames(campath_mod, np_wad, size):
        if "light_bands" not in notes:
            continue
        with np.errstate(all="ignore"):
            z = np.array([nm.f_as_i16(k["GCFX"] * np.float32(notes["wz"]) / (k["CFY"] - np.float32(y))) for y in range(H)])
        far, near = z == 32767, z == -32768
        assert far.sum() >= 2 and near.sum() >= 2
        lit = lambda light, rows: want[rows][:, notes["light_bands"][light]].any()
        assert not lit(1784, far) and not lit(-32768, far) and not lit(-32768, near)
        assert lit(2042, far) and lit(32767, far)
        assert all(lit(light, near) for light in rc.LIGHTS[1:])


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fpx", ["0", "1"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_gpu_equals_independent_restatement(dg, wad1993, campath_mod, np_wad, monkeypatch, size, fpx):
    """All cases of a size in ONE dg_draw_lists batch, then in reverse order, against the numpy frames pixel for pixel."""
    W, H = size
    exp = expected_frames(campath_mod, np_wad, size)
    monkeypatch.setenv("DOOMGPU_FRAME_PER_XCD", fpx)                          # read by every raster launch
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=len(exp), slots=1)
    ctx.upload_scene(scene)
    try:
        lists = [to_dg_lists(dg, scene, rec, l) for _, rec, l, _, _ in exp]
        t0 = time.perf_counter()
        for label, idx in (("in order", list(range(len(exp)))), ("reversed", list(range(len(exp)))[::-1])):
            out = ctx.draw_lists(0, (dg.DgFrameLists * len(idx))(*[lists[i][0] for i in idx]))
            for j, i in enumerate(idx):
                _diff(out[j], exp[i][4], f"{exp[i][0]} ({label}, frame {j}, {W}x{H}, frame_per_xcd {fpx})")
        print(f"raster classes {W}x{H} frame_per_xcd {fpx}: {len(exp)} frames x 2 in {time.perf_counter() - t0:.3f} s")
    finally:
        ctx.close()
        scene.close()
