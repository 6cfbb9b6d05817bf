"""The tile rasteriser's fixed-shape bodies for wave-tiles whose eight columns all have a sole plain owner (kernels.hip strip_body).

A wave-tile is what one wavefront renders of one 64 x 64 tile: the eight columns x0 + wave + 8k.  strip_body takes a body of its own when
all eight have a sole plain owner of one kind (eight walls, or eight floors / ceilings) — "clean" when nothing is laid on top of any of them,
"lean" when every possibly-transparent span left by the pre-filter is a plain wall covering all live rows — and the general pipeline for every
other wave-tile, the few whose eight sole owners are of both kinds included.  Pixels must not change.
  CPU tier: the views below, grouped into wave-tiles through the observer (emul_bind.EmulScene.observe_lists), hold every kind of wave-tile the
            choice distinguishes — so the GPU tier cannot pass without entering the new bodies and without leaving them where it must.
  GPU tier: the same views through the host-list front end and through the device column walk, DOOMGPU_FRAME_PER_XCD 0 and 1, byte for byte
            against the CPU oracle; and one batch of nine frames (a frame beyond the last multiple of eight keeps dispatch order).
Sizes: 256x192; 200x136 (a partial strip and a packed last tile row); 72x100 (an eight-column second strip: its waves have ONE column inside
the frame — the kernel runs them with nk == WAVES and seven empty columns, which must fall to the general code); 70x96 (a width that is not a
multiple of 4: dg_raster_tiles_anyw).
"""
import itertools

import numpy as np
import pytest

import emul_bind
from emul_bind import OV_HIT, PATH_MASK, PATHS

VIEWS = [0, 100, 297, 323, 500, 623, 728, 900]
SIZES = [(256, 192), (200, 136), (72, 100), (70, 96)]
IDS = [f"{w}x{h}" for w, h in SIZES]
KINDS = ("clean", "sole_with_overlays", "mixed_kinds", "seven_of_eight", "partial_all_sole", "packed")
SPAN_CAP = 512                       # kernels.hip: a strip with more spans is staged in rounds of whole columns
SOLE = (PATHS["SOLE_WALL"], PATHS["SOLE_FLAT"])

_ORACLE = {}


def oracle_frames(oracle_scene1993, path1993, size, views=tuple(VIEWS)):
    """The CPU oracle's frames of a size, rendered once for all GPU tests."""
    key = (size, views)
    if key not in _ORACLE:
        W, H = size
        _ORACLE[key] = [np.frombuffer(oracle_scene1993.render(W, H, path1993[i]), dtype=np.uint8).reshape(H, W, 3) for i in views]
    return _ORACLE[key]


def staging_rounds(lcoff):
    """The column ranges [c_lo, c_hi) one strip is staged in (strip_body's `while (c_lo < TILE_W)` loop head): all 64 columns when their spans
    fit the staging area, else as many whole columns at a time as fit.  lcoff: the 65 span offsets of the strip's columns."""
    rounds, c_lo = [], 0
    while c_lo < 64:
        c_hi = 64
        if lcoff[64] - lcoff[0] > SPAN_CAP and lcoff[64] - lcoff[c_lo] > SPAN_CAP:
            c_hi = c_lo + 1
            while c_hi < 64 and lcoff[c_hi + 1] - lcoff[c_lo] <= SPAN_CAP:
                c_hi += 1
        rounds.append((c_lo, c_hi))
        c_lo = c_hi
    return rounds


def wave_tile_kinds(obs, W, H):
    """Counts of the wave-tile kinds in one observed frame."""
    count = dict.fromkeys(KINDS, 0)
    col_off = np.concatenate([[0], np.cumsum(np.bincount(obs["spans"][:, 0].astype(np.int64), minlength=W))])
    for x0 in range(0, W, 64):
        for c_lo, c_hi in staging_rounds([int(col_off[min(x0 + c, W)]) for c in range(65)]):
            for ty, wave in itertools.product(range((H + 63) // 64), range(8)):
                cols = [x0 + c for c in range(c_lo + wave, c_hi, 8) if x0 + c < W]
                codes = [int(obs["chunks"][ty, x]) for x in cols]
                if not codes:
                    continue
                sole = [(c & PATH_MASK) in SOLE for c in codes]
                clean = [s and not c & OV_HIT for s, c in zip(sole, codes)]
                if any((c & PATH_MASK) == PATHS["PACKED"] for c in codes):
                    count["packed"] += 1
                elif len(cols) < 8:
                    count["partial_all_sole"] += all(sole)
                elif all(sole) and len({c & PATH_MASK for c in codes}) == 2:
                    count["mixed_kinds"] += 1
                elif all(clean):
                    count["clean"] += 1
                elif all(sole):
                    count["sole_with_overlays"] += 1
                elif sum(clean) == 7 and sum(sole) == 7:
                    count["seven_of_eight"] += 1
    return count


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------

def test_the_views_hold_every_kind_of_wave_tile(dg, wad1993, path1993):
    scene, emul = dg.Scene(wad1993, "e1m1"), emul_bind.EmulScene(wad1993)
    total = {}
    try:
        for W, H in SIZES:
            count = dict.fromkeys(KINDS, 0)
            for view in dg.make_views(path1993[VIEWS]):
                fl = scene.build_lists(W, H, view)
                for kind, n in wave_tile_kinds(emul.observe_lists(W, H, fl), W, H).items():
                    count[kind] += n
            total[(W, H)] = count
    finally:
        scene.close()
    print(total)
    for kind in KINDS:
        assert sum(c[kind] for c in total.values()) > 0, (kind, total)
    assert total[(256, 192)]["clean"] > 0 and total[(256, 192)]["sole_with_overlays"] > 0 and total[(256, 192)]["seven_of_eight"] > 0
    assert total[(200, 136)]["packed"] > 0 and total[(72, 100)]["partial_all_sole"] > 0
    assert total[(70, 96)]["clean"] > 0                                      # dg_raster_tiles_anyw enters the new body too


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------

def _render_and_compare(dg, wad1993, path1993, want, size, views, front_end, label):
    W, H = size
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=len(views), slots=1, front_end=front_end)
    ctx.upload_scene(scene)
    try:
        out = ctx.render(dg.make_views(path1993[list(views)]))
        for k, i in enumerate(views):
            bad = np.argwhere(np.any(out[k] != want[k], axis=-1))
            assert len(bad) == 0, f"{label}: view {i} (frame {k}): {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"
    finally:
        ctx.close()
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fpx", ["0", "1"])
@pytest.mark.parametrize("front_end", ["host", "device"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_gpu_frames_equal_the_oracle(dg, wad1993, path1993, oracle_scene1993, monkeypatch, size, front_end, fpx):
    monkeypatch.setenv("DOOMGPU_FRAME_PER_XCD", fpx)                          # read by every raster launch
    want = oracle_frames(oracle_scene1993, path1993, size)
    fe = dg.DG_FE_HOST if front_end == "host" else dg.DG_FE_DEVICE
    _render_and_compare(dg, wad1993, path1993, want, size, VIEWS, fe, f"{size[0]}x{size[1]} {front_end} front end, frame_per_xcd {fpx}")


@pytest.mark.gpu
@pytest.mark.parametrize("fpx", ["0", "1"])
def test_gpu_batch_of_nine_frames(dg, wad1993, path1993, oracle_scene1993, monkeypatch, fpx):
    """Eight frames go to one XCD each, the ninth keeps dispatch order (raster_block)."""
    monkeypatch.setenv("DOOMGPU_FRAME_PER_XCD", fpx)
    views = tuple(VIEWS + [150])
    want = oracle_frames(oracle_scene1993, path1993, (256, 192), views)
    _render_and_compare(dg, wad1993, path1993, want, (256, 192), views, dg.DG_FE_HOST, f"nine frames, frame_per_xcd {fpx}")
