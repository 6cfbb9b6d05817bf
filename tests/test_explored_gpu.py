"""GPU tier of the explored-map frames.

1. dg_seen_lines_device between torch tensors against the numpy restatement (np_explored): synthetic planes at four sizes (one and two
   bands, a run across a band edge), a base off the 16-byte boundary, a map with more than 4 096 segs, the error returns, slots in flight
   left alone — in ONE child process (tests/explored/torch_cases.py), because torch has to be imported before libdoomgpu.so is loaded.
2. dg_slot_seen_lines of a label slot and of a bundle slot equals the host entries on the slot's own planes: sub-ranges, run lengths, the
   carry chained over two submissions, each output left out, what other slots are refused.
3. Explored map frames equal dg_explored_map_host at every store form, with the masks of the CPU tier; all ones equals render_map; the
   slot machinery; a new upload rebuilds the cover; an explored and a 3-D submission in flight together.
4. End to end: a walk turning on the spot -> label frames -> dg_slot_seen_lines -> explored frames, against the model on host planes.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import explored_cases as xc
import np_automap as na
import np_explored as ne

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_CASES = [f"synthetic/{W}x{H}" for W, H in ((64, 40), (131, 67), (5, 9), (96, 200))] + ["unaligned", "many_segs", "errors", "in_flight"]


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/explored/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("explored") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "explored", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


@pytest.mark.parametrize("case", TORCH_CASES)
def test_seen_lines_device(torch_cases, case):
    assert torch_cases[case] == "ok"


# ---- dg_slot_seen_lines --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def light(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc, ne.Explored(wad1993)
    sc.close()


def _same_outputs(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("kind", ["labels", "bundle"])
def test_slot_seen_lines_equals_the_host_entries(dg, light, path1993, kind):
    sc, ex = light
    W, H, n = 320, 200, 16
    ctx = dg.Context(W, H, max_batch=3 * n, slots=2)
    ctx.upload_scene(sc)
    submit = (lambda slot, v: ctx.submit_labels(slot, v)) if kind == "labels" else (lambda slot, v: ctx.submit_bundle(slot, v, dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_LABELS))
    first, second = dg.make_views(path1993[0:960:60]), dg.make_views(path1993[30:990:60])
    submit(0, first)
    ids, cls, _ = ctx.readback_labels(0, 0, n)
    seen = dg.seen_lines_host(sc, ids, cls)
    assert np.array_equal(seen, ex.seen(ids, cls)) and seen.any()
    rng = np.random.default_rng(7)
    for run_len in (1, 4, 16):
        runs = n // run_len
        for carry in (None, rng.integers(0, 1 << 32, (runs, ex.words), dtype=np.uint64).astype(np.uint32) & seen[3]):
            _same_outputs(ctx.slot_seen_lines(0, 0, n, run_len, carry), dg.seen_accumulate_host(seen, run_len, carry), (run_len, carry is not None))
    t = ctx.seen_kernel_ms()
    assert t["lines_ms"] > 0.0 and t["accumulate_ms"] > 0.0, t
    for lo, count, run_len in ((3, 8, 4), (15, 1, 1), (0, 0, 1), (5, 6, 3)):
        _same_outputs(ctx.slot_seen_lines(0, lo, count, run_len), dg.seen_accumulate_host(seen[lo:lo + count], run_len), (lo, count, run_len))
    whole = dg.seen_accumulate_host(seen, 4)
    for k in dg.SEEN_OUTPUTS:                                              # each output alone, and each left out
        _same_outputs(ctx.slot_seen_lines(0, 0, n, 4, want=(k,)), {k: whole[k]}, k)
        rest = tuple(j for j in dg.SEEN_OUTPUTS if j != k)
        _same_outputs(ctx.slot_seen_lines(0, 0, n, 4, want=rest), {j: whole[j] for j in rest}, rest)
    assert ctx.slot_seen_lines(0, 0, n, 4, want=()) == {}
    # the carry chained over two submissions equals one run of the concatenation
    a = ctx.slot_seen_lines(0, 0, n, n)
    submit(1, second)
    b = ctx.slot_seen_lines(1, 0, n, n, a["carry_out"])
    ids2, cls2, _ = ctx.readback_labels(1, 0, n)
    both = dg.seen_accumulate_host(np.concatenate([seen, dg.seen_lines_host(sc, ids2, cls2)]), 2 * n)
    assert np.array_equal(np.concatenate([a["upto"], b["upto"]]), both["upto"]) and np.array_equal(b["carry_out"], both["carry_out"])
    assert np.array_equal(np.concatenate([a["total"], b["total"]]), both["total"]) and np.array_equal(np.concatenate([a["fresh"], b["fresh"]]), both["fresh"])
    # the planes stay as they are
    again = ctx.readback_labels(0, 0, n)
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], cls)
    # what is refused
    L = dg.lib()
    call = lambda slot, lo, count, run_len: L.dg_slot_seen_lines(ctx._h, slot, lo, count, run_len, None, None, None, None, None)
    for args in ((0, -1, 1, 1), (0, 0, -1, 1), (0, 10, 7, 1), (0, 0, 16, 0), (0, 0, 16, -1), (0, 0, 16, 5), (2, 0, 1, 1), (-1, 0, 1, 1)):
        assert call(*args) == dg.DG_ERR_INVALID, args
    assert call(0, 0, 16, 16) == dg.DG_OK
    ctx.close()


def test_slot_seen_lines_refuses_slots_without_label_planes(dg, light, path1993):
    sc, ex = light
    ctx = dg.Context(320, 200, max_batch=12, slots=1)
    L = dg.lib()
    call = lambda: L.dg_slot_seen_lines(ctx._h, 0, 0, 1, 1, None, None, None, None, None)
    assert call() == dg.DG_ERR_INVALID                                       # nothing uploaded, an empty slot
    ctx.upload_scene(sc)
    assert call() == dg.DG_ERR_INVALID
    v = dg.make_views(path1993[100:104])
    ones = np.tile(ex.bits_to_row(range(ex.n_lines)), (4, 1))
    for submit in (lambda: ctx.submit(0, v), lambda: ctx.submit_depth(0, v), lambda: ctx.submit_map(0, v), lambda: ctx.submit_explored_map(0, v, ones),
                   lambda: ctx.submit_bundle(0, v, dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH)):
        submit()
        assert call() == dg.DG_ERR_INVALID
        ctx.wait(0)
    ctx.submit_labels(0, v)
    assert call() == dg.DG_OK
    ctx.close()


# ---- explored map frames -------------------------------------------------------------------------------------------------------------------------

def _host_frames(dg, sc, W, H, views, masks):
    return np.stack([dg.explored_map_host(sc, W, H, v, m) for v, m in zip(views, masks)])


@pytest.fixture(scope="module")
def light_masks(dg, light, path1993):
    """The masks of the CPU tier for the light map: frame_masks plus the seen rows of two path views."""
    sc, ex = light
    seen = dg.seen_lines_host(sc, *xc.path_label_planes(dg, sc, 160, 100, dg.make_views(path1993[[0, 623]])))
    return xc.frame_masks(ex, extra_rows=[seen[0], seen[0] | seen[1]])


@pytest.mark.parametrize("size", [(64, 40), (44, 41), (131, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_explored_frames_equal_the_host_rule(dg, light, light_masks, path1993, size):
    """64x40: the 16-byte store form, 44x41: the 12-byte form, 131x67: the byte form — one batch, another mask and view per frame."""
    sc, ex = light
    W, H = size
    assert ((3 * W * H) % 16 == 0, (3 * W * H) % 4 == 0) == {(64, 40): (True, True), (44, 41): (False, True), (131, 67): (False, False)}[size]
    names, masks = list(light_masks), np.stack(list(light_masks.values()))
    n = len(names)
    views = dg.make_views(path1993[np.arange(n) * 37 % 1000])
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(sc)
    got = ctx.render_explored_map(views, masks)
    want = _host_frames(dg, sc, W, H, views, masks)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), (names[k], int((got[k] != want[k]).any(axis=2).sum()))
    t = ctx.timing(0)
    assert t["front_end"] == dg.DG_FE_MAP_EXPLORED and t["n_frames"] == n and t["setup_ms"] > 0 and t["raster_ms"] > 0       # this submission uploaded the cover
    # all ones == the map view's bytes
    ones = np.tile(light_masks["all_ones"], (n, 1))
    assert np.array_equal(ctx.render_explored_map(views, ones), ctx.render_map(views))
    # ... and the model, for the frames where the topmost line at the vertex is missing
    for k, name in enumerate(names):
        if name.startswith("without_") or name.startswith("only_"):
            rec = path1993[k * 37 % 1000]
            assert np.array_equal(got[k], ex.frame(W, H, na.path_view(rec), masks[k])), name
    ctx.close()


def test_one_frame_at_1280x800(dg, light, light_masks, path1993):
    sc, ex = light
    W, H = 1280, 800
    ctx = dg.Context(W, H, max_batch=2, slots=1)
    ctx.upload_scene(sc)
    views = dg.make_views(path1993[[500, 728]])
    masks = np.stack([light_masks["extra_1"], light_masks["without_" + "_".join(map(str, xc.meeting_lines(ex)[-1:]))]])
    got = ctx.render_explored_map(views, masks)
    assert np.array_equal(got, _host_frames(dg, sc, W, H, views, masks))
    assert np.array_equal(ctx.render_explored_map(views, np.tile(light_masks["all_ones"], (2, 1))), ctx.render_map(views))
    ctx.close()


def test_batches_replay_async_readback_and_checksums(dg, light, light_masks, path1993):
    sc, ex = light
    W, H, F = 320, 200, 24
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(sc)
    rows = np.stack(list(light_masks.values()))
    fallbacks = ctx.fallbacks()
    for n, first in ((1, 5), (9, 100), (F, 700)):
        views = dg.make_views(path1993[first:first + n])
        masks = rows[(np.arange(n) * 5 + n) % len(rows)]
        got = ctx.render_explored_map(views, masks)
        assert np.array_equal(got, _host_frames(dg, sc, W, H, views, masks)), n
    assert ctx.timing(0)["setup_ms"] == 0.0                                   # the cover was there
    n = 9
    views, masks = dg.make_views(path1993[200:200 + n]), rows[np.arange(n) * 3 % len(rows)]
    want = _host_frames(dg, sc, W, H, views, masks)
    ctx.submit_explored_map(1, views, masks)
    masks[:] = 0                                                              # the call copied them
    host = dg.lib().dg_alloc_host(n * 3 * W * H)
    try:
        ctx.readback_async(1, 0, n, host)
        ctx.wait(1)
        got = np.ctypeslib.as_array((ctypes.c_uint8 * (n * 3 * W * H)).from_address(host)).reshape(n, H, W, 3).copy()
    finally:
        dg.lib().dg_free_host(host)
    assert np.array_equal(got, want)
    sums = ctx.frame_checksums(1, 0, n)
    assert list(sums) == [dg.frame_checksum(w) for w in want]
    # another submission in the other slot, then a replay of this one: the slot kept its mask rows
    ctx.submit_explored_map(0, dg.make_views(path1993[:F]), np.zeros((F, ex.words), np.uint32))
    fb = ctx.framebuffer_ptr(1)
    ctx.replay(1)
    ctx.wait(1)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP_EXPLORED and t["setup_ms"] == 0.0 and t["raster_ms"] > 0 and t["total_ms"] == t["raster_ms"]
    assert ctx.framebuffer_ptr(1) == fb and list(ctx.frame_checksums(1, 0, n)) == list(sums)
    assert np.array_equal(ctx.readback(1, 0, n), want)
    assert np.array_equal(ctx.readback_reduced(1, 0, n, (4, 4)), dg.reduce_host(want, (4, 4)))
    assert ctx.fallbacks() == fallbacks
    ctx.close()


def test_second_upload_rebuilds_the_cover(dg, synth, wad1993, wad1995, path1993):
    W, H = 320, 200
    ctx = dg.Context(W, H, max_batch=4, slots=1)
    views = dg.make_views(path1993[:4])
    scenes = []
    for wad in (wad1993, wad1995, wad1993):
        sc, ex = dg.Scene(wad, "e1m1"), ne.Explored(wad)
        scenes.append(sc)
        ctx.upload_scene(sc)
        rng = np.random.default_rng(ex.n_lines)
        masks = rng.integers(0, 1 << 32, (4, ex.words), dtype=np.uint64).astype(np.uint32)
        masks[:, -1] &= np.uint32((1 << (ex.n_lines % 32)) - 1) if ex.n_lines % 32 else np.uint32(0xFFFFFFFF)
        got = ctx.render_explored_map(views, masks)
        assert ctx.timing(0)["setup_ms"] > 0
        assert np.array_equal(got, _host_frames(dg, sc, W, H, views, masks))
        assert np.array_equal(got[0], ex.frame(W, H, na.path_view(path1993[0]), masks[0]))
    ctx.close()
    for sc in scenes:
        sc.close()


def test_an_explored_and_a_3d_submission_in_flight(dg, oracle, light, wad1993, path1993):
    sc, ex = light
    W, H = 320, 200
    osc = oracle.Scene(wad1993, "e1m1")
    idx = [0, 100, 297, 323, 500, 623, 728, 900]
    recs = path1993[idx]
    v = dg.make_views(recs)
    rng = np.random.default_rng(3)
    masks = rng.integers(0, 1 << 32, (8, ex.words), dtype=np.uint64).astype(np.uint32) & ex.bits_to_row(range(ex.n_lines))
    want3d = [dg.frame_checksum(osc.render(W, H, r)) for r in recs]
    wantmap = [dg.frame_checksum(f) for f in _host_frames(dg, sc, W, H, v, masks)]
    ctx = dg.Context(W, H, max_batch=8, slots=2)
    ctx.upload_scene(sc)
    for first, second in (("3d", "map"), ("map", "3d")):
        for slot, what in enumerate((first, second)):
            ctx.submit(slot, v) if what == "3d" else ctx.submit_explored_map(slot, v, masks)
        ctx.wait(0)
        ctx.wait(1)
        a, b = list(ctx.frame_checksums(0, 0, 8)), list(ctx.frame_checksums(1, 0, 8))
        assert (a, b) == ((want3d, wantmap) if first == "3d" else (wantmap, want3d))
    # one slot: 3-D, explored, map, explored
    ctx.submit(0, v)
    ctx.submit_explored_map(0, v, masks)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap
    ctx.submit_map(0, v)
    assert ctx.timing(0)["front_end"] == dg.DG_FE_MAP
    ctx.submit_explored_map(0, v, masks)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap and ctx.timing(0)["front_end"] == dg.DG_FE_MAP_EXPLORED
    ctx.close()


def test_explored_error_returns(dg, light, wad1993):
    sc, ex = light
    L = dg.lib()
    v = (dg.DgView * 4)(*[dg.DgView(1000.0, 1000.0, 0.5, 0, 0, 0, 0, 0, 0, 0)] * 4)
    ones = np.tile(ex.bits_to_row(range(ex.n_lines)), (4, 1))
    P = ones.ctypes.data_as(dg._P)
    ctx = dg.Context(320, 200, max_batch=3, slots=1)
    assert L.dg_submit_explored_map_views(ctx._h, 0, v, 1, P) == dg.DG_ERR_INVALID          # no scene uploaded
    ctx.upload_scene(sc)
    assert L.dg_submit_explored_map_views(ctx._h, 0, v, 4, P) == dg.DG_ERR_CAPACITY         # n > max_batch
    assert L.dg_submit_explored_map_views(ctx._h, 0, v, 0, P) == dg.DG_ERR_CAPACITY
    assert L.dg_submit_explored_map_views(ctx._h, 1, v, 1, P) == dg.DG_ERR_INVALID          # slot out of range
    assert L.dg_submit_explored_map_views(ctx._h, 0, v, 1, None) == dg.DG_ERR_INVALID       # NULL mask
    assert L.dg_render_explored_map_views(ctx._h, None, 1, P, None) == dg.DG_ERR_INVALID
    far = (dg.DgView * 1)(dg.DgView(1e12, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
    assert L.dg_submit_explored_map_views(ctx._h, 0, far, 1, P) == dg.DG_ERR_INVALID        # arrow beyond +-2^24
    assert ctx.render_explored_map((dg.DgView * 3)(*v[:3]), ones[:3]).any()                  # still usable
    ctx.close()
    # more than 65 536 linedefs: a mask row would not fit the frame kernel's staging
    many = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 2, 14, 65537), "e1m1")
    assert dg.seen_words(many) == 2049
    wide = np.zeros((1, 2049), np.uint32)
    big = dg.Context(320, 200, max_batch=1, slots=1)
    big.upload_scene(many)
    assert L.dg_submit_explored_map_views(big._h, 0, v, 1, wide.ctypes.data_as(dg._P)) == dg.DG_ERR_CAPACITY
    assert L.dg_render_explored_map_views(big._h, v, 1, wide.ctypes.data_as(dg._P), None) == dg.DG_ERR_CAPACITY
    assert big.render_map((dg.DgView * 1)(v[0])).any()                                       # the map view itself has no such limit
    big.close()
    many.close()
    small = dg.Context(39, 40, max_batch=1, slots=1)
    small.upload_scene(sc)
    assert L.dg_submit_explored_map_views(small._h, 0, v, 1, P) == dg.DG_ERR_INVALID
    small.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------

def test_a_walk_that_turns_on_the_spot_reveals_the_map(dg, light):
    sc, ex = light
    W, H, tics = 320, 200, 24
    walk = dg.Walk(sc, np.full(tics, dg.DG_KEY_LEFT, np.uint8))
    views = walk.views((np.arange(tics + 1) + 0.5) / 35.0)
    n = len(views)
    ctx = dg.Context(W, H, max_batch=n, slots=2)
    ctx.upload_scene(sc)
    ctx.submit_labels(0, views)
    acc = ctx.slot_seen_lines(0, 0, n, n)
    got = ctx.render_explored_map(views, acc["upto"])
    # the model, from the host label planes alone
    ids, cls = xc.path_label_planes(dg, sc, W, H, views)
    want = ne.accumulate(ex.seen(ids, cls), n)
    for k in dg.SEEN_OUTPUTS:
        assert np.array_equal(acc[k], want[k]), k
    for f in (0, n // 2, n - 1):
        rv = (np.float32(views[f].x), np.float32(views[f].y), np.float32(views[f].angle), np.float32(views[f].cos_a), np.float32(views[f].sin_a))
        assert np.array_equal(got[f], ex.frame(W, H, rv, want["upto"][f])), f
    assert np.array_equal(got, _host_frames(dg, sc, W, H, views, want["upto"]))
    assert acc["total"][-1] > acc["total"][0] > 0 and acc["fresh"][1:].sum() == acc["total"][-1] - acc["total"][0]
    lines = lambda f: ((f[..., 0] == 255) & (f[..., 2] == 0)).sum()
    assert lines(ctx.render_explored_map(views, acc["upto"])[-1]) > 0
    first_only, last_only = (dg.explored_map_host(sc, W, H, None, acc["upto"][k]) for k in (0, n - 1))
    assert lines(last_only) > lines(first_only)                              # the last frame shows strictly more of the map
    walk.close()
    ctx.close()
