"""GPU tier of the player-centred map frames: dg_ego_tiles against dg_ego_map_host, byte for byte (the host entry is held against the
numpy restatement by tests/test_ego_host.py).

A band is rows = max(1, 8192 // W) whole rows, the resolve phase stores 16 pixels, 4 pixels or 1 pixel per item (ego_core.h):
   64x40     one band, 16-byte stores
   44x41     dword stores (by rows = 8192 // 44 = 186 the frame is ONE band; 300x41 below is the dword form with two bands)
   300x41    dword stores, two bands (27 rows, then 14)
   131x67    byte stores, two bands (62 rows, then 5)
   320x200   eight bands of 25 rows, 16-byte stores
   1280x800  6-row bands, the last of 2 rows
Every size runs submissions that between them mix the scales, both rotate settings, mask rows and the NULL mask, arrow on and off (one
dg_ego_map holds for a submission, so the mix is over submissions; the masks differ per frame).  The kernel examines the linedefs in
chunks of CHUNK = 256 (EGO_CHUNK), which is also its survivor list's capacity: test_more_lines_in_a_band_than_a_chunk_holds.
"""
import ctypes

import numpy as np
import pytest

import explored_cases as xc
import np_ego as ng
import np_explored as ne

pytestmark = pytest.mark.gpu

CHUNK = 256
R, A = ng.ROTATE, ng.ARROW
CONFIGS = [(2.0 ** -10, 0, False), (0.05, R | A, True), (1.0, A, True), (8.0, R, False), (64.0, R | A, True), (0.25, R | A, True), (4.0, 0, True)]
SHAPES = {(64, 40): (1, 16), (44, 41): (1, 4), (300, 41): (2, 4), (131, 67): (2, 1), (320, 200): (8, 16), (1280, 800): (134, 16)}   # (bands, pixels per store item)


def _shape(W, H):
    rows = max(1, 8192 // W)
    bands = -(-H // rows)
    ok = lambda m: (W * H) % m == 0 and (bands == 1 or (W * rows) % m == 0)
    return bands, 16 if ok(16) else 4 if ok(4) else 1


@pytest.fixture(scope="module")
def light(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc, ng.EgoModel(wad1993)
    sc.close()


def _mask_rows(model, n, seed):
    """n rows: random halves, all ones, all zero, one line."""
    rng = np.random.default_rng(seed)
    ones = model.bits_to_row(range(model.n_lines))
    rows = (rng.integers(0, 1 << 32, (n, model.words), dtype=np.uint64).astype(np.uint32)) & ones
    rows[1 % n] = ones
    rows[2 % n] = 0
    rows[3 % n] = model.bits_to_row([model.n_lines // 2])
    return rows


def _host(dg, sc, W, H, views, params, masks):
    return np.stack([dg.ego_map_host(sc, W, H, v, params, None if masks is None else masks[k]) for k, v in enumerate(views)])


def _check_configs(dg, ctx, sc, model, path, W, H, n, configs=CONFIGS):
    lit = 0
    for k, (scale, flags, masked) in enumerate(configs):
        views = dg.make_views(path[(np.arange(n) * 37 + 100 * k) % 1000])
        masks = _mask_rows(model, n, k) if masked else None
        got = ctx.render_ego_map(views, (scale, flags), masks)
        want = _host(dg, sc, W, H, views, (scale, flags), masks)
        for f in range(n):
            assert np.array_equal(got[f], want[f]), (W, H, scale, flags, masked, f, int((got[f] != want[f]).any(axis=2).sum()))
        lit += int(want.any())
    assert lit >= len(configs) - 2


@pytest.mark.parametrize("size", [(64, 40), (44, 41), (300, 41), (131, 67), (320, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_host_rule(dg, light, path1993, size):
    sc, model = light
    W, H = size
    assert _shape(W, H) == SHAPES[size]
    ctx = dg.Context(W, H, max_batch=6, slots=1)
    ctx.upload_scene(sc)
    _check_configs(dg, ctx, sc, model, path1993, W, H, 6)
    # one frame against the numpy restatement itself
    v = dg.make_views(path1993[[500]])
    row = _mask_rows(model, 1, 9)
    got = ctx.render_ego_map(v, (0.25, R | A), row)
    assert np.array_equal(got[0], model.frame(W, H, ng.view_of(v[0]), 0.25, R | A, row[0]))
    ctx.close()


def test_three_frames_at_1280x800(dg, light, path1993):
    sc, model = light
    W, H = 1280, 800
    assert _shape(W, H) == SHAPES[(W, H)] and H % 6 == 2
    ctx = dg.Context(W, H, max_batch=3, slots=1)
    ctx.upload_scene(sc)
    _check_configs(dg, ctx, sc, model, path1993, W, H, 3, [(0.25, R | A, True), (4.0, A, False), (64.0, R, True)])
    ctx.close()


def test_batches_of_1_9_and_max_batch(dg, light, path1993):
    sc, model = light
    W, H, F = 64, 40, 24
    ctx = dg.Context(W, H, max_batch=F, slots=1)
    ctx.upload_scene(sc)
    for n in (1, 9, F):
        _check_configs(dg, ctx, sc, model, path1993, W, H, n, [(0.25, R | A, True), (1.0, 0, False)])
    ctx.close()


def test_more_lines_in_a_band_than_a_chunk_holds(dg, wad1994, path1994):
    """At scale 2^-10 every drawn line of the level lies within a pixel of the centre, at 0.004 the whole level sits inside the one band of a 64x40
    frame: every line survives the clip, and a level with more than CHUNK lines fills the survivor list chunk after chunk."""
    sc, model = dg.Scene(wad1994, "e1m1"), ng.EgoModel(wad1994)
    drawn = sum(1 for _, _, fl in model.lines if not fl & 128)
    assert drawn > 2 * CHUNK and drawn % CHUNK != 0
    W, H = 64, 40
    ctx = dg.Context(W, H, max_batch=4, slots=1)
    ctx.upload_scene(sc)
    views = dg.make_views(path1994[[0, 300, 600, 900]])
    for scale, flags in ((2.0 ** -10, 0), (2.0 ** -10, R | A), (0.004, R), (0.02, A)):
        for masks in (None, _mask_rows(model, 4, 5)):
            got = ctx.render_ego_map(views, (scale, flags), masks)
            assert np.array_equal(got, _host(dg, sc, W, H, views, (scale, flags), masks)), (scale, flags, masks is None)
    ctx.close()
    sc.close()


def test_timing_async_readback_checksums_reduced_and_replay(dg, light, path1993):
    sc, model = light
    W, H, F = 320, 200, 12
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(sc)
    fallbacks = ctx.fallbacks()
    n = 9
    views = dg.make_views(path1993[200:200 + n])
    masks = _mask_rows(model, n, 3)
    params = dg.DgEgoMap(0.25, R | A)
    want = _host(dg, sc, W, H, views, params, masks)
    ctx.submit_ego_map(1, views, params, masks)
    # the call copied what it needs: the caller's arrays may go
    masks[:] = 0xFFFFFFFF
    params.scale, params.flags = 7.0, 0
    ctypes.memset(views, 0, ctypes.sizeof(views))
    host = dg.lib().dg_alloc_host(n * 3 * W * H)
    try:
        ctx.readback_async(1, 0, n, host)
        ctx.wait(1)
        got = np.ctypeslib.as_array((ctypes.c_uint8 * (n * 3 * W * H)).from_address(host)).reshape(n, H, W, 3).copy()
    finally:
        dg.lib().dg_free_host(host)
    assert np.array_equal(got, want)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP_EGO and t["n_frames"] == n and t["setup_ms"] > 0 and t["raster_ms"] > 0     # this submission uploaded the table
    sums = ctx.frame_checksums(1, 0, n)
    assert list(sums) == [dg.frame_checksum(w) for w in want]
    # another ego submission in the other slot (no mask, no arrow), then a replay of this one: the slot kept views, arrow and mask rows
    other = dg.make_views(path1993[:F])
    ctx.submit_ego_map(0, other, (1.0, 0))
    fb = ctx.framebuffer_ptr(1)
    ctx.replay(1)
    ctx.wait(1)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP_EGO and t["setup_ms"] == 0.0 and t["raster_ms"] > 0 and t["total_ms"] == t["raster_ms"]
    assert ctx.framebuffer_ptr(1) == fb and list(ctx.frame_checksums(1, 0, n)) == list(sums)
    assert np.array_equal(ctx.readback(1, 0, n), want)
    assert np.array_equal(ctx.readback_reduced(1, 0, n, (4, 4)), dg.reduce_host(want, (4, 4)))
    assert np.array_equal(ctx.readback(0, 0, F), _host(dg, sc, W, H, other, (1.0, 0), None))
    assert ctx.timing(0)["setup_ms"] == 0.0                                   # the table was there
    # a masked submission after an unmasked one in the same slot, and the other way round
    views = dg.make_views(path1993[200:200 + n])
    m2 = _mask_rows(model, n, 4)
    ctx.submit_ego_map(0, views, (0.25, A), m2)
    assert np.array_equal(ctx.readback(0, 0, n), _host(dg, sc, W, H, views, (0.25, A), m2))
    ctx.submit_ego_map(0, views, (0.25, A))
    assert np.array_equal(ctx.readback(0, 0, n), _host(dg, sc, W, H, views, (0.25, A), None))
    assert ctx.fallbacks() == fallbacks
    ctx.close()


def test_second_upload_rebuilds_the_table(dg, wad1993, wad1995, path1993):
    W, H = 320, 200
    ctx = dg.Context(W, H, max_batch=4, slots=1)
    views = dg.make_views(path1993[[0, 300, 600, 900]])
    scenes = []
    for wad in (wad1993, wad1995, wad1993):
        sc, model = dg.Scene(wad, "e1m1"), ng.EgoModel(wad)
        scenes.append(sc)
        ctx.upload_scene(sc)
        masks = _mask_rows(model, 4, model.n_lines)
        got = ctx.render_ego_map(views, (0.125, R | A), masks)
        assert ctx.timing(0)["setup_ms"] > 0
        assert np.array_equal(got, _host(dg, sc, W, H, views, (0.125, R | A), masks)) and got.any()
        assert np.array_equal(ctx.render_ego_map(views, (0.125, 0)), _host(dg, sc, W, H, views, (0.125, 0), None))
        assert ctx.timing(0)["setup_ms"] == 0.0
    ctx.close()
    for sc in scenes:
        sc.close()


def test_an_ego_and_a_3d_submission_in_flight(dg, oracle, light, wad1993, path1993):
    sc, model = light
    W, H = 320, 200
    osc = oracle.Scene(wad1993, "e1m1")
    recs = path1993[[0, 100, 297, 323, 500, 623, 728, 900]]
    v = dg.make_views(recs)
    masks = _mask_rows(model, 8, 11)
    p = (0.25, R | A)
    want3d = [dg.frame_checksum(osc.render(W, H, r)) for r in recs]
    wantmap = [dg.frame_checksum(f) for f in _host(dg, sc, W, H, v, p, masks)]
    ctx = dg.Context(W, H, max_batch=8, slots=2)
    ctx.upload_scene(sc)
    for first, second in (("3d", "map"), ("map", "3d")):
        for slot, what in enumerate((first, second)):
            ctx.submit(slot, v) if what == "3d" else ctx.submit_ego_map(slot, v, p, masks)
        ctx.wait(0)
        ctx.wait(1)
        a, b = list(ctx.frame_checksums(0, 0, 8)), list(ctx.frame_checksums(1, 0, 8))
        assert (a, b) == ((want3d, wantmap) if first == "3d" else (wantmap, want3d))
    # one slot: 3-D, ego, map, explored, ego
    ctx.submit(0, v)
    ctx.submit_ego_map(0, v, p, masks)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap
    ctx.submit_map(0, v)
    assert ctx.timing(0)["front_end"] == dg.DG_FE_MAP
    ctx.submit_explored_map(0, v, masks)
    assert ctx.timing(0)["front_end"] == dg.DG_FE_MAP_EXPLORED
    ctx.submit_ego_map(0, v, p, masks)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap and ctx.timing(0)["front_end"] == dg.DG_FE_MAP_EGO
    ctx.close()


def test_error_returns_through_the_ctx(dg, light, wad1993):
    sc, model = light
    L = dg.lib()
    v = (dg.DgView * 4)(*[dg.DgView(1000.0, 1000.0, 0.5, 0, 0, 0, 0, 0, 0, 0)] * 4)
    ones = np.tile(model.bits_to_row(range(model.n_lines)), (4, 1))
    P = ones.ctypes.data_as(dg._P)
    good = dg.DgEgoMap(1.0, R | A)
    g = ctypes.byref(good)
    ctx = dg.Context(320, 200, max_batch=3, slots=1)
    assert L.dg_submit_ego_map_views(ctx._h, 0, v, 1, g, P) == dg.DG_ERR_INVALID             # no scene uploaded
    ctx.upload_scene(sc)
    assert L.dg_submit_ego_map_views(ctx._h, 0, v, 4, g, P) == dg.DG_ERR_CAPACITY            # n > max_batch
    assert L.dg_submit_ego_map_views(ctx._h, 0, v, 0, g, P) == dg.DG_ERR_CAPACITY
    assert L.dg_submit_ego_map_views(ctx._h, 1, v, 1, g, P) == dg.DG_ERR_INVALID             # slot out of range
    assert L.dg_submit_ego_map_views(ctx._h, 0, None, 1, g, P) == dg.DG_ERR_INVALID
    assert L.dg_submit_ego_map_views(ctx._h, 0, v, 1, None, P) == dg.DG_ERR_INVALID
    assert L.dg_render_ego_map_views(ctx._h, None, 1, g, P, None) == dg.DG_ERR_INVALID
    for bad in (dg.DgEgoMap(0.0, 0), dg.DgEgoMap(65.0, 0), dg.DgEgoMap(float("nan"), 0), dg.DgEgoMap(1.0, 4)):
        assert L.dg_submit_ego_map_views(ctx._h, 0, v, 1, ctypes.byref(bad), P) == dg.DG_ERR_INVALID
    # a view out of contract: the frame index is in the message
    mixed = (dg.DgView * 3)(v[0], v[1], dg.DgView(1e6, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
    assert L.dg_submit_ego_map_views(ctx._h, 0, mixed, 3, g, P) == dg.DG_ERR_INVALID and b"frame 2" in L.dg_last_error()
    mixed[2] = dg.DgView(0.0, 0.0, 0.0, 0, 2.0, 0.0, 0, 0, 0, 1)
    assert L.dg_submit_ego_map_views(ctx._h, 0, mixed, 3, g, P) == dg.DG_ERR_INVALID and b"frame 2" in L.dg_last_error()
    assert ctx.render_ego_map((dg.DgView * 3)(*v[:3]), good, ones[:3]).any()                  # still usable
    ctx.close()
    many = dg.Scene(xc.grow_map_lump(wad1993, "E1M1", 2, 14, 65536), "e1m1")
    big = dg.Context(320, 200, max_batch=1, slots=1)
    big.upload_scene(many)
    assert L.dg_submit_ego_map_views(big._h, 0, v, 1, g, None) == dg.DG_ERR_CAPACITY
    assert L.dg_render_ego_map_views(big._h, v, 1, g, None, None) == dg.DG_ERR_CAPACITY
    big.close()
    many.close()
    small = dg.Context(15, 40, max_batch=1, slots=1)
    small.upload_scene(sc)
    assert L.dg_submit_ego_map_views(small._h, 0, v, 1, g, None) == dg.DG_ERR_INVALID
    small.close()


def test_a_walk_that_turns_on_the_spot_reveals_the_map_around_the_player(dg, light, wad1993):
    sc, model = light
    ex = ne.Explored(wad1993)
    W, H, tics = 320, 200, 24
    walk = dg.Walk(sc, np.full(tics, dg.DG_KEY_LEFT, np.uint8))
    views = walk.views((np.arange(tics + 1) + 0.5) / 35.0)
    n = len(views)
    ctx = dg.Context(W, H, max_batch=n, slots=2)
    ctx.upload_scene(sc)
    ctx.submit_labels(0, views)
    acc = ctx.slot_seen_lines(0, 0, n, n)
    p = (0.125, A)                                                           # north up: the frames of a turn on the spot differ by what was seen (and the arrow)
    got = ctx.render_ego_map(views, p, acc["upto"])
    # the model, from the host label planes alone
    ids, cls = xc.path_label_planes(dg, sc, W, H, views)
    want = ne.accumulate(ex.seen(ids, cls), n)
    assert np.array_equal(acc["upto"], want["upto"])
    for f in (0, n // 2, n - 1):
        assert np.array_equal(got[f], model.frame(W, H, ng.view_of(views[f]), *p, want["upto"][f])), f
    assert np.array_equal(got, _host(dg, sc, W, H, views, p, want["upto"]))
    lit = lambda f: int(f.any(axis=2).sum())
    no_arrow = ctx.render_ego_map(views, (0.125, 0), acc["upto"])
    assert lit(no_arrow[-1]) > lit(no_arrow[0]) > 0 and lit(got[-1]) > lit(got[0])
    walk.close()
    ctx.close()
