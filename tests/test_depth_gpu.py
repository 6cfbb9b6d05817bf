"""GPU tier of the depth / surface-kind frame: dg_depth_tiles through the ctx entry points against dg_depth_lists_host (which the CPU
tier, test_depth_host.py, holds against the np_depth model), byte for byte.

  hand-built lists   tests/depth_cases.py at 64x40 (one strip), 131x67 (partial strip, odd W*H), 5x9 (narrower than a wave) and 320x200
                     (several strips, a short last row band: 200 = 128 + 72): the 70-span column, 24 spans on every column (more than the
                     16 the kernel stages in LDS); fetched through dg_readback_depth with sub-ranges and with either output NULL
  views              dg_render_depth_views == the host function on dg_build_lists output: 16 path frames at 320x200 and 2 at 1280x800 on
                     the light map, 8 at 320x200 on the heavy map, on ctxs of every front end; with per-view states that change a sprite
                     frame; with wall effects and map-object thinkers on
  pipelining         a depth slot and a colour slot in flight together
  slot rules         colour after depth and depth after colour, the refused calls, dg_slot_timing, a pending dg_readback_async, the
                     fallback counters
  plane layout       the slab behind dg_slot_framebuffer for n = 3 at 5x9
"""
import ctypes

import numpy as np
import pytest

import depth_cases
import mobj_fx as mf
from test_edge_kats import to_dg_lists, view_dict

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


def _same(got, want, what):
    for name, g, w in (("distance", got[0], want[0]), ("kind", got[1], want[1])):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} pixels differ, first at {bad[0].tolist()}: gpu {g[tuple(bad[0])]} host {w[tuple(bad[0])]}"


def _host_of_views(dg, scene, W, H, views):
    """dg_depth_lists_host on dg_build_lists output, one view at a time (the lists live in a per-thread arena)."""
    d = np.empty((len(views), H, W), dtype=np.int16)
    k = np.empty((len(views), H, W), dtype=np.uint8)
    for i in range(len(views)):
        frames = (dg.DgFrameLists * 1)(scene.build_lists(W, H, views[i]))
        d[i], k[i] = [p[0] for p in dg.depth_lists_host(scene, W, H, frames)]
    return d, k


@pytest.fixture(scope="module")
def scene1993(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def scene1994(dg, wad1994):
    sc = dg.Scene(wad1994, "e1m1")
    yield sc
    sc.close()


@pytest.mark.parametrize("size", [(64, 40), (131, 67), (5, 9), (320, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hand_built_lists_equal_the_host_function(dg, campath_mod, scene1993, size):
    W, H = size
    cs = depth_cases.cases(W, H)
    keep, frames = [], (dg.DgFrameLists * len(cs))()
    for i, (name, v, lists) in enumerate(cs):
        rec, _vd = view_dict(campath_mod, *v)
        frames[i], k = to_dg_lists(dg, scene1993, rec, lists)
        keep.append(k)
    want = dg.depth_lists_host(scene1993, W, H, frames)
    assert all((want[1][i] != 0).any() for i in range(len(cs)))
    n = len(cs)
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scene1993)
    assert dg.lib().dg_depth_lists(ctx._h, 0, frames, n, None, None) == dg.DG_OK          # neither output: the call only waits
    _same(ctx.readback_depth(0, 0, n), want, f"{W}x{H}")
    d, k = ctx.readback_depth(0, 1, n - 1, kind=False)
    assert k is None and np.array_equal(d, want[0][1:])
    d, k = ctx.readback_depth(0, n - 1, 1, distance=False)
    assert d is None and np.array_equal(k, want[1][n - 1:])
    assert dg.lib().dg_readback_depth(ctx._h, 0, 2, 0, None, None) == dg.DG_OK           # count = 0 does nothing
    for (first, count) in ((-1, 1), (0, n + 1), (n, 1), (0, -1)):
        assert dg.lib().dg_readback_depth(ctx._h, 0, first, count, None, None) == dg.DG_ERR_INVALID
    _same(ctx.depth_lists(0, frames), want, f"{W}x{H} again")                              # the synchronous call with both outputs
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEPTH
    ctx.close()
    del keep


@pytest.fixture(scope="module")
def view_batches(dg, scene1993, scene1994, path1993, path1994):
    """[(what, scene, W, H, views, host planes)] — the host planes computed once for the three front ends."""
    out = []
    for what, sc, W, H, recs in (("light 320x200", scene1993, 320, 200, path1993[0:960:60]), ("light 1280x800", scene1993, 1280, 800, path1993[[297, 728]]),
                                 ("heavy 320x200", scene1994, 320, 200, path1994[0:1000:125])):
        views = dg.make_views(recs)
        out.append((what, sc, W, H, views, _host_of_views(dg, sc, W, H, views)))
    assert [len(b[4]) for b in out] == [16, 2, 8]
    return out


@pytest.mark.parametrize("front_end", [1, 2, 3], ids=["host-lists", "device-column-walk", "device-seg-walk"])
def test_views_equal_the_host_function_whatever_the_front_end(dg, view_batches, front_end):
    for what, sc, W, H, views, want in view_batches:
        ctx = dg.Context(W, H, max_batch=len(views), slots=1, front_end=front_end)
        ctx.upload_scene(sc)
        _same(ctx.render_depth(views), want, f"{what} front end {front_end}")
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEPTH
        assert {1, 2, 3} <= set(np.unique(want[1]).tolist())
        assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
        ctx.close()


def test_per_view_states_that_change_a_sprite_frame(dg, wad1993, path1993):
    """Every view carries a snapshot that gives a third of the map objects another sprite (or none); the host planes come from a second
    scene object with the same states set on the scene itself."""
    W, H = 320, 200
    idx = [0, 100, 297, 323, 500, 623, 728, 900]
    sc = dg.Scene(wad1993, "e1m1")
    names = [None, "BAR1", "POSS", "TROO", "COLU", "TRED"]
    handles = {n: sc.sprite_frame(n, 0) for n in names if n}
    rng = np.random.default_rng(7)
    views = dg.make_views(path1993[idx])
    states = []
    want_d, want_k = np.empty((len(idx), H, W), np.int16), np.empty((len(idx), H, W), np.uint8)
    for k in range(len(idx)):
        ref = dg.Scene(wad1993, "e1m1")
        for n in names[1:]:
            ref.sprite_frame(n, 0)                                   # the same bitmaps decoded in the same order: the same ids
        mobjs = []
        for m in rng.choice(ref.mobj_count(), size=ref.mobj_count() // 3, replace=False):
            name = names[int(rng.integers(len(names)))]
            fb = bool(rng.integers(2))
            mobjs.append((int(m), -1 if name is None else handles[name], int(fb)))
            ref.set_mobj_state(int(m), name, 0, fb)
        states.append(([], mobjs))
        d, kd = _host_of_views(dg, ref, W, H, views[k:k + 1])
        want_d[k], want_k[k] = d[0], kd[0]
        ref.close()
    plain = _host_of_views(dg, sc, W, H, views)
    assert not np.array_equal(plain[0], want_d)                      # the states show in the distance plane
    ctx = dg.Context(W, H, max_batch=len(idx), slots=1, front_end=3)
    ctx.upload_scene(sc)
    st, keep = dg.make_view_states(states)
    _same(ctx.render_depth(views, st), (want_d, want_k), "per-view states")
    _same(ctx.render_depth(views), plain, "no states")
    ctx.close()
    sc.close()
    del keep


def test_wall_effects_and_map_object_thinkers_on(dg, path1993):
    W, H = 320, 200
    sc = dg.Scene(mf.fx_wad(), "E1M1")
    sc.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    sc.mobj_event(dg.DG_MOBJ_KILL, mf.ts(140))
    idx = [0, 54, 140, 266, 404, 541, 703, 879]
    views = dg.make_views(path1993[idx])
    for k, T in enumerate((1, 7, 139, 141, 148, 160, 200, 300)):
        views[k].timestamp = mf.ts(T)
    want = _host_of_views(dg, sc, W, H, views)                       # dg_build_lists draws with the scene's effects at each view's timestamp
    still = dg.make_views(path1993[idx])
    assert not np.array_equal(_host_of_views(dg, sc, W, H, still)[0], want[0])    # the timestamps show
    ctx = dg.Context(W, H, max_batch=len(idx), slots=1, front_end=3)
    ctx.upload_scene(sc)
    _same(ctx.render_depth(views), want, "effects on")
    ctx.close()
    sc.close()


def test_a_depth_slot_and_a_colour_slot_in_flight_together(dg, scene1993, path1993, view_batches):
    what, sc, W, H, views, want = view_batches[0]
    ctx = dg.Context(W, H, max_batch=len(views), slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    ctx.submit(1, views)
    ctx.wait(1)
    alone = ctx.frame_checksums(1, 0, len(views))
    ctx.submit(1, views)
    ctx.submit_depth(0, views)
    ctx.submit(1, views)                                             # a second colour batch behind the depth kernel
    ctx.wait(0)
    ctx.wait(1)
    assert np.array_equal(ctx.frame_checksums(1, 0, len(views)), alone)
    _same(ctx.readback_depth(0, 0, len(views)), want, "depth next to colour")
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    ctx.close()


def test_slot_rules(dg, scene1993, path1993, view_batches):
    what, sc, W, H, views, want = view_batches[0]
    n = len(views)
    L = dg.lib()
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    colour = ctx.render(views)
    assert L.dg_readback_depth(ctx._h, 0, 0, 1, None, None) == dg.DG_ERR_INVALID         # the last submission is colour
    assert L.dg_readback_depth(ctx._h, 1, 0, 0, None, None) == dg.DG_ERR_INVALID         # ... or nothing at all
    # a depth submission on a slot with a pending dg_readback_async completes that readback first
    nbytes = n * ctx.frame_bytes
    buf = L.dg_alloc_host(nbytes)
    host = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    host[:] = 0xA5
    ctx.submit(0, views)
    ctx.readback_async(0, 0, n, buf)
    ctx.submit_depth(0, views)
    assert np.array_equal(host.reshape(colour.shape), colour)
    _same(ctx.readback_depth(0, 0, n), want, "depth after colour")
    t = ctx.timing(0)
    assert t["front_end"] == dg.DG_FE_DEPTH and t["n_frames"] == n and t["raster_ms"] > 0 and t["setup_ms"] == 0
    # the calls that would read the planes as RGB24, or run the colour kernels on the slot again
    out = np.zeros(nbytes, dtype=np.uint8)
    desc = dg.DgReduceDesc(2, 2, 0, 0)
    sums = np.zeros(n, dtype=np.uint64)
    refused = [L.dg_readback(ctx._h, 0, 0, 1, out.ctypes.data_as(P)), L.dg_readback_async(ctx._h, 0, 0, 1, P(buf)),
               L.dg_readback_reduced(ctx._h, 0, 0, 1, ctypes.byref(desc), out.ctypes.data_as(P)),
               L.dg_readback_reduced_async(ctx._h, 0, 0, 1, ctypes.byref(desc), P(buf)),
               L.dg_frame_checksums(ctx._h, 0, 0, 1, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), L.dg_replay_slot(ctx._h, 0)]
    assert refused == [dg.DG_ERR_INVALID] * 6
    assert b"depth" in L.dg_last_error()
    assert not out.any() and not sums.any()
    ctx.wait(0)
    _same(ctx.readback_depth(0, 0, n), want, "after the refused calls")
    assert isinstance(ctx.framebuffer_ptr(0), int)
    # a colour submission into the slot that held depth
    ctx.submit(0, views)
    assert np.array_equal(ctx.readback(0, 0, n), colour)
    assert ctx.timing(0)["front_end"] == 2
    assert L.dg_readback_depth(ctx._h, 0, 0, 1, None, None) == dg.DG_ERR_INVALID
    # dg_upload_scene on a ctx with a depth slot in flight
    ctx.submit_depth(1, views)
    ctx.upload_scene(scene1993)
    assert L.dg_readback_depth(ctx._h, 1, 0, 1, None, None) == dg.DG_ERR_INVALID         # every slot is empty after an upload
    _same(ctx.render_depth(views), want, "after the upload")
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    # errors of the submission itself
    assert L.dg_submit_depth_views(ctx._h, 0, None, None, n) == dg.DG_ERR_INVALID
    assert L.dg_submit_depth_views(ctx._h, 2, views, None, n) == dg.DG_ERR_INVALID
    assert L.dg_submit_depth_views(ctx._h, 0, views, None, n + 1) == dg.DG_ERR_CAPACITY
    assert L.dg_depth_lists(ctx._h, 0, None, 1, None, None) == dg.DG_ERR_INVALID
    L.dg_free_host(buf)
    ctx.close()


def test_plane_layout_in_the_framebuffer_slab(dg, campath_mod, scene1993):
    """n = 3 at 5x9: int16 distance[3][9][5] at the slab's base, uint8 kind[3][9][5] at byte offset 2 * 3 * 45.  The slab's 3 * n * W * H raw
    bytes are copied, device to device, into a finished colour slot (dg_reduce_device with 1x1 boxes is a copy) and read from there."""
    W, H, n = 5, 9, 3
    cs = depth_cases.cases(W, H)[:n]
    keep, frames = [], (dg.DgFrameLists * n)()
    for i, (name, v, lists) in enumerate(cs):
        rec, _vd = view_dict(campath_mod, *v)
        frames[i], k = to_dg_lists(dg, scene1993, rec, lists)
        keep.append(k)
    want = dg.depth_lists_host(scene1993, W, H, frames)
    ctx = dg.Context(W, H, max_batch=n, slots=2)
    ctx.upload_scene(scene1993)
    ctx.draw_lists(1, frames)                                        # slot 1: a finished colour submission of n frames
    ctx.depth_lists(0, frames)
    ctx.reduce_device(ctx.framebuffer_ptr(0), W, H, n, (1, 1), ctx.framebuffer_ptr(1))
    raw = ctx.readback(1, 0, n).reshape(-1)
    assert raw.size == 3 * n * W * H
    assert np.array_equal(raw[:2 * n * W * H].view("<i2").reshape(n, H, W), want[0])
    assert np.array_equal(raw[2 * n * W * H:].reshape(n, H, W), want[1])
    ctx.close()
    del keep
