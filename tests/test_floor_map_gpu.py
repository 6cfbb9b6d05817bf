"""GPU tier of the floor-textured player-centred map frames: dg_floor_map_tiles (and, with a mask, dg_floor_seen_sectors) against
dg_floor_map_host, byte for byte — the host entry is held against the numpy restatement by tests/test_floor_map_host.py.

The band decomposition and the store forms are dg_ego_tiles' (tests/test_ego_gpu.py):
   64x40     one band, 16-byte stores              44x41     dword stores, one band
   300x41    dword stores, two bands               131x67    byte stores, two bands
   320x200   eight bands, 16-byte stores           1280x800  6-row bands, the last of 2 rows
Pixel centres within a rounding of a partition line, exactly on it, on segs and vertices, and the contract's corners (scales 2^-10 and 64,
|view| 65536, 16384x16) are held against the host and the numpy model (floor_map_cases.WITNESS_CASES, TIE_CASES, CORNER_CASES).
Every size runs every case of floor_map_cases.py as a submission of three frames (the case's view moved along x, a mask row of its own
per frame, the case's light and flat entries in the first and the last frame): masks, states, surfaces, the light effects, animated flats and
a sky floor are among the cases.  Frames narrower or lower than 16 pixels (8200x2, and the 65 537 frames of 4x1 that cross the grid's y
extent) are below the C-ABI's contract: tests/floor_map/floor_map_launch_main.hip drives the launcher itself with them.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import floor_map_cases as fc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORLDS = ("light", "hand", "hand_sky")
SHAPES = {(64, 40): (1, 16), (44, 41): (1, 4), (300, 41): (2, 4), (131, 67): (2, 1), (320, 200): (8, 16), (1280, 800): (134, 16)}   # (bands, pixels per store item)


def _shape(W, H):
    rows = max(1, 8192 // W)
    bands = -(-H // rows)
    ok = lambda m: (W * H) % m == 0 and (bands == 1 or (W * rows) % m == 0)
    return bands, 16 if ok(16) else 4 if ok(4) else 1


@pytest.fixture(scope="module")
def scenes(dg):
    out = {w: fc.open_scene(dg, w) for w in WORLDS}
    assert out["light"].use_picture("BON1A0") == 0                            # (before any upload: a screen picture for the overlay)
    yield out
    for sc in out.values():
        sc.close()


def _batch(dg, sc, c, n):
    """n frames of case c: (views, mask rows or None, states or None, surfaces or None) as lists per frame."""
    views = (dg.DgView * n)()
    for k in range(n):
        x, y, a = c["view"]
        views[k] = dg.DgView(x + 16.5 * k, y - 3.25 * k, a + 0.01 * k, 0, 0, 0, 0, 0, c["ts"] + 0.35 * k, 0)
    masks = None if c["mask"] is None else np.stack([fc.mask_row(c, k) for k in range(n)])
    with_entries = lambda k: k == 0 or k == n - 1
    states = None if not c["lights"] else [fc.state_of(c) if with_entries(k) else ([], []) for k in range(n)]
    surfaces = None if not c["flats"] else [fc.surfaces_of(sc, c) if with_entries(k) else ([], []) for k in range(n)]
    return views, masks, states, surfaces


def _host(dg, sc, W, H, c, batch):
    views, masks, states, surfaces = batch
    return np.stack([dg.floor_map_host(sc, W, H, views[k], (c["scale"], c["flags"]), None if masks is None else masks[k], None if states is None else states[k],
                                       None if surfaces is None else surfaces[k]) for k in range(len(views))])


def _check_case(dg, ctx, sc, c, W, H, n):
    batch = _batch(dg, sc, c, n)
    views, masks, states, surfaces = batch
    got = ctx.render_floor_map(views, (c["scale"], c["flags"]), masks, states, surfaces)
    want = _host(dg, sc, W, H, c, batch)
    for f in range(n):
        assert np.array_equal(got[f], want[f]), (c["name"], W, H, f, int((got[f] != want[f]).any(axis=2).sum()))
    return want


def _check_world(dg, scenes, world, W, H, n, cases=None):
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scenes[world])
    lit = 0
    for c in (cases if cases is not None else [c for c in fc.CASES if c["world"] == world]):
        lit += int(_check_case(dg, ctx, scenes[world], c, W, H, n).any())
    ctx.close()
    assert lit > 0


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("size", [(64, 40), (44, 41), (300, 41), (131, 67), (320, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_host_rule(dg, scenes, size, world):
    W, H = size
    assert _shape(W, H) == SHAPES[size]
    _check_world(dg, scenes, world, W, H, 3)


def test_one_frame_against_the_numpy_model(dg, scenes):
    W, H = 131, 67
    for name in ("light_masked_half", "hand_entries", "sky_floor"):
        c = fc.BY_NAME[name]
        sc = scenes[c["world"]]
        ctx = dg.Context(W, H, max_batch=1, slots=1)
        ctx.upload_scene(sc)
        m = fc.mask_row(c)
        got = ctx.render_floor_map((dg.DgView * 1)(fc.view_of(dg, c)), (c["scale"], c["flags"]), None if m is None else m[None, :],
                                   None if not c["lights"] else [fc.state_of(c)], None if not c["flats"] else [fc.surfaces_of(sc, c)])
        assert np.array_equal(got[0], fc.model_frame(c, W, H)), name
        ctx.close()


def _render_cases(dg, ctx, sc, cases):
    """The cases' own views as one submission: they share scale and flags; a mask row, if any has one, per frame."""
    c0 = cases[0]
    assert all((c["scale"], c["flags"], c["world"]) == (c0["scale"], c0["flags"], c0["world"]) and not c["lights"] and not c["flats"] for c in cases)
    views = (dg.DgView * len(cases))(*[fc.view_of(dg, c) for c in cases])
    masks = None if c0["mask"] is None else np.stack([fc.mask_row(c) for c in cases])
    return ctx.render_floor_map(views, (c0["scale"], c0["flags"]), masks)


def _check_against_host_and_model(dg, sc, cases, W, H, what):
    ctx = dg.Context(W, H, max_batch=len(cases), slots=1)
    ctx.upload_scene(sc)
    got = _render_cases(dg, ctx, sc, cases)
    ctx.close()
    for k, c in enumerate(cases):
        host = dg.floor_map_host(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c))
        want = fc.model_frame(c, W, H)
        assert want.any()
        print(f"{what} {c['name']} {W}x{H}: {int((got[k] != host).any(axis=2).sum())} pixels differ from the host's, {int((got[k] != want).any(axis=2).sum())} from the model's")
        assert np.array_equal(got[k], host) and np.array_equal(got[k], want), (what, c["name"], W, H)


@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_witnesses_of_a_fused_side_test(dg, scenes, size):
    """floor_map_cases.WITNESS_CASES as one batch: pixel centres at which the rule's side test is 0.0 and a fused one is not (the import
    asserts what a fused model draws there), and the rotated view of which a fused rotation changes 16 pixels and more at 320x200.  A
    library built with contraction on fails here."""
    _check_against_host_and_model(dg, scenes["hand"], fc.WITNESS_CASES, *size, "witness")
    _check_against_host_and_model(dg, scenes["light"], [fc.ROTATION_WITNESS], *size, "witness")


@pytest.mark.parametrize("size", fc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixel_centres_exactly_on_partition_segs_and_vertices(dg, scenes, size):
    """floor_map_cases.TIE_CASES: the descent's <= and floor_behind's < where the test is exactly 0.0."""
    for c in fc.TIE_CASES:
        _check_against_host_and_model(dg, scenes["hand"], [c], *size, "tie")


@pytest.mark.parametrize("c", fc.CORNER_CASES, ids=lambda c: c["name"])
def test_the_corners_of_the_contract(dg, scenes, c):
    _check_against_host_and_model(dg, scenes[c["world"]], [c], *c["size"], "corner")


def test_the_wave_shapes_the_cases_name(dg, scenes):
    """floor_map_cases asserts at import which waves occur in WAVE_CASES at 131x67, cut as the kernel cuts them: no wanting lane, the
    first wanting lane in the upper half, only lane 63, a partial last wave, whole waves past the band, parting at the root and at the
    last node above the leaves."""
    for name in fc.WAVE_CASES:
        c = fc.BY_NAME[name]
        _check_against_host_and_model(dg, scenes[c["world"]], [c], 131, 67, "waves")


def test_three_frames_at_1280x800(dg, scenes):
    W, H = 1280, 800
    assert _shape(W, H) == SHAPES[(W, H)] and H % 6 == 2
    _check_world(dg, scenes, "light", W, H, 3, [fc.BY_NAME[n] for n in ("light_masked_half", "light_entries", "light_close")])
    _check_world(dg, scenes, "hand_sky", W, H, 3, [fc.BY_NAME["sky_floor"]])


def test_batches_of_1_9_and_max_batch(dg, scenes):
    W, H, F = 64, 40, 24
    sc = scenes["light"]
    ctx = dg.Context(W, H, max_batch=F, slots=1)
    ctx.upload_scene(sc)
    for n in (1, 9, F):
        for name in ("light_masked_half", "light_entries", "light_unit_1"):
            _check_case(dg, ctx, sc, fc.BY_NAME[name], W, H, n)
    ctx.close()


def test_the_launcher_past_the_grid_extent_and_on_the_wide_tile(tmp_path):
    """tests/floor_map/floor_map_launch_main.hip: launch_floor_map_tiles itself on a two-room scene built in the program — 65 537 frames of
    4x1 (two launches: the grid's y extent is 65 535), 8200x2 (the wide tile, one row per band) and 300x41 with a mask through
    dg_floor_seen_sectors — against the host loop over the same shared functions.  It checks its own results."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "floor_map_launch_main"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
                           "-o", str(exe), os.path.join(HERE, "floor_map", "floor_map_launch_main.hip"), os.path.join(csrc, "floor_map_kernels.hip")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "floor_map_launch_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_kernel_on_tables_no_map_has_and_on_indices_it_must_refuse(tmp_path):
    """tests/floor_map/floor_map_tables_main.hip: dg_floor_map_tiles on tables built in the program (floor_map_tables.h) — no nodes, a leaf
    without a sector, a leaf without segs, a chain of 200 partitions, and a child, leaf, sector, seg range and flat out of range, each on
    device tables whose slack holds decoys that would light the pixel — against the rule's functions on the host.  It checks its own
    results."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "floor_map_tables_main"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
                           "-o", str(exe), os.path.join(HERE, "floor_map", "floor_map_tables_main.hip"), os.path.join(csrc, "floor_map_kernels.hip")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "floor_map_tables_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_timing_readbacks_overlay_and_replay(dg, scenes):
    sc = scenes["light"]
    W, H, F = 320, 200, 8
    c = fc.BY_NAME["light_masked_half"]
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(sc)
    fallbacks = ctx.fallbacks()
    n = 6
    batch = _batch(dg, sc, c, n)
    views, masks, states, surfaces = batch
    params = dg.DgEgoMap(c["scale"], c["flags"])
    want = _host(dg, sc, W, H, c, batch)
    ctx.submit_floor_map(1, views, params, masks)
    sent = np.array(masks)
    masks[:] = 0xFFFFFFFF                                                     # the call copied what it needs: the caller's arrays may go
    params.scale, params.flags = 7.0, 0
    host = dg.lib().dg_alloc_host(n * 3 * W * H)
    try:
        ctx.readback_async(1, 0, n, host)
        ctx.wait(1)
        got = np.ctypeslib.as_array((ctypes.c_uint8 * (n * 3 * W * H)).from_address(host)).reshape(n, H, W, 3).copy()
    finally:
        dg.lib().dg_free_host(host)
    assert np.array_equal(got, want)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP_FLOOR and t["n_frames"] == n and t["setup_ms"] > 0 and t["raster_ms"] > 0       # this submission uploaded the tables
    sums = ctx.frame_checksums(1, 0, n)
    assert list(sums) == [dg.frame_checksum(w) for w in want]
    # an ego submission in the other slot finds its line table there; a replay of this one: the slot kept views, arrow, mask rows and cells
    ctx.submit_ego_map(0, views, (1.0, 0))
    ctx.wait(0)
    assert ctx.timing(0)["setup_ms"] == 0.0
    ctx.replay(1)
    ctx.wait(1)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP_FLOOR and t["setup_ms"] == 0.0 and t["raster_ms"] > 0 and t["total_ms"] == t["raster_ms"]
    assert list(ctx.frame_checksums(1, 0, n)) == list(sums)
    assert np.array_equal(ctx.readback(1, 0, n), want)
    assert np.array_equal(ctx.readback_reduced(1, 0, n, (4, 4)), dg.reduce_host(want, (4, 4)))
    # screen pictures over a floor-map slot; dg_slot_seen_lines refuses it
    items = [[(0, 10 + 3 * f, 20, 2, 2, 200, 0)] for f in range(n)]
    ctx.slot_overlay(1, 0, items)
    over = dg.overlay_host(sc, want.copy(), items)
    assert np.array_equal(ctx.readback(1, 0, n), over) and not np.array_equal(over, want)
    with pytest.raises(dg.DoomGpuError) as e:
        ctx.slot_seen_lines(1, 0, n, n)
    assert e.value.code == dg.DG_ERR_INVALID
    # a masked submission after an unmasked one in the same slot, and the other way round
    ctx.submit_floor_map(0, views, (c["scale"], c["flags"]))
    assert np.array_equal(ctx.readback(0, 0, n), _host(dg, sc, W, H, c, (views, None, None, None)))
    ctx.submit_floor_map(0, views, (c["scale"], c["flags"]), sent)
    assert np.array_equal(ctx.readback(0, 0, n), want)
    assert ctx.fallbacks() == fallbacks
    ctx.close()


def test_second_upload_rebuilds_the_tables(dg, scenes):
    W, H = 320, 200
    ctx = dg.Context(W, H, max_batch=3, slots=1)
    for world, name in (("hand", "hand_whole"), ("light", "light_masked_half"), ("hand_sky", "sky_floor"), ("hand", "hand_room_a_only")):
        ctx.upload_scene(scenes[world])
        c = fc.BY_NAME[name]
        assert _check_case(dg, ctx, scenes[world], c, W, H, 3).any()
        assert ctx.timing(0)["setup_ms"] > 0
        _check_case(dg, ctx, scenes[world], c, W, H, 2)
        assert ctx.timing(0)["setup_ms"] == 0.0
    ctx.close()


def test_a_floor_map_and_a_3d_submission_in_flight(dg, oracle, wad1993, path1993):
    W, H = 320, 200
    sc = dg.Scene(wad1993, "e1m1")
    osc = oracle.Scene(wad1993, "e1m1")
    recs = path1993[[0, 100, 297, 323, 500, 623, 728, 900]]
    v = dg.make_views(recs)
    p = (0.25, fc.R | fc.A)
    want3d = [dg.frame_checksum(osc.render(W, H, r)) for r in recs]
    wantmap = [dg.frame_checksum(dg.floor_map_host(sc, W, H, v[k], p)) for k in range(8)]
    ctx = dg.Context(W, H, max_batch=8, slots=2)
    ctx.upload_scene(sc)
    for first, second in (("3d", "map"), ("map", "3d")):
        for slot, what in enumerate((first, second)):
            ctx.submit(slot, v) if what == "3d" else ctx.submit_floor_map(slot, v, p)
        ctx.wait(0)
        ctx.wait(1)
        a, b = list(ctx.frame_checksums(0, 0, 8)), list(ctx.frame_checksums(1, 0, 8))
        assert (a, b) == ((want3d, wantmap) if first == "3d" else (wantmap, want3d))
    # one slot: 3-D, floor map, ego, floor map
    ctx.submit(0, v)
    ctx.submit_floor_map(0, v, p)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap
    ctx.submit_ego_map(0, v, p)
    assert ctx.timing(0)["front_end"] == dg.DG_FE_MAP_EGO
    ctx.submit_floor_map(0, v, p)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap and ctx.timing(0)["front_end"] == dg.DG_FE_MAP_FLOOR
    ctx.close()
    sc.close()


def test_error_returns_through_the_ctx(dg, scenes):
    sc = scenes["hand"]
    L = dg.lib()
    v = (dg.DgView * 4)(*[dg.DgView(352.5, 250.0, 0.5, 0, 0, 0, 0, 0, 0, 0)] * 4)
    good = dg.DgEgoMap(0.25, fc.R | fc.A)
    g = ctypes.byref(good)
    ctx = dg.Context(320, 200, max_batch=3, slots=1)
    sub = lambda *a: L.dg_submit_floor_map_views(ctx._h, *a)
    assert sub(0, v, 1, g, None, None, None) == dg.DG_ERR_INVALID                              # no scene uploaded
    ctx.upload_scene(sc)
    keep = ctx.render_floor_map((dg.DgView * 3)(*v[:3]), good)
    sums = list(ctx.frame_checksums(0, 0, 3))

    def refused(rc, want=dg.DG_ERR_INVALID):                                                 # ... and the slot holds what it held
        assert rc == want and list(ctx.frame_checksums(0, 0, 3)) == sums and ctx.timing(0)["front_end"] == dg.DG_FE_MAP_FLOOR, rc

    refused(sub(0, v, 4, g, None, None, None), dg.DG_ERR_CAPACITY)                            # n > max_batch
    refused(sub(0, v, 0, g, None, None, None), dg.DG_ERR_CAPACITY)
    assert sub(1, v, 1, g, None, None, None) == dg.DG_ERR_INVALID                             # slot out of range
    refused(sub(0, None, 1, g, None, None, None))
    refused(sub(0, v, 1, None, None, None, None))
    assert L.dg_render_floor_map_views(ctx._h, None, 1, g, None, None, None, None) == dg.DG_ERR_INVALID
    for bad in (dg.DgEgoMap(0.0, 0), dg.DgEgoMap(65.0, 0), dg.DgEgoMap(float("nan"), 0), dg.DgEgoMap(1.0, 4)):
        refused(sub(0, v, 1, ctypes.byref(bad), None, None, None))
    mixed = (dg.DgView * 3)(v[0], v[1], dg.DgView(1e6, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
    refused(sub(0, mixed, 3, g, None, None, None))
    assert b"frame 2" in L.dg_last_error()
    mixed[2] = dg.DgView(0.0, 0.0, 0.0, 0, 2.0, 0.0, 0, 0, 0, 1)
    refused(sub(0, mixed, 3, g, None, None, None))
    # a view's state and surfaces: the third frame's entry is out of range
    st, k1 = dg.make_view_states([([(0, 100)], []), ([], []), ([(2, 100)], [])])
    refused(sub(0, v, 3, g, None, st, None))
    assert b"frame 2" in L.dg_last_error()
    loaded = sc.sector_flats()
    sf, k2 = dg.make_view_surfaces([([], []), ([], [(0, 0x0FFFFFF, int(loaded[0][2]))]), ([], [])])
    refused(sub(0, v, 3, g, None, None, sf))
    assert b"frame 1" in L.dg_last_error()
    null_flats = (dg.DgViewSurfaces * 3)(dg.DgViewSurfaces(None, 0, None, 0), dg.DgViewSurfaces(None, 0, None, 0), dg.DgViewSurfaces(None, 0, None, 2))
    refused(sub(0, v, 3, g, None, None, null_flats))
    null_lights = (dg.DgViewState * 3)(dg.DgViewState(None, 1, None, 0), dg.DgViewState(None, 0, None, 0), dg.DgViewState(None, 0, None, 0))
    refused(sub(0, v, 3, g, None, null_lights, None))
    assert np.array_equal(ctx.readback(0, 0, 3), keep)
    assert np.array_equal(ctx.render_floor_map((dg.DgView * 3)(*v[:3]), good), keep)            # still usable
    ctx.close()
    small = dg.Context(15, 40, max_batch=1, slots=1)
    small.upload_scene(sc)
    assert L.dg_submit_floor_map_views(small._h, 0, v, 1, g, None, None, None) == dg.DG_ERR_INVALID
    small.close()
