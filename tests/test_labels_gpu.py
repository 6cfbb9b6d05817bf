"""GPU tier of the object-label frame: dg_label_tiles and dg_label_boxes through the ctx entry points against dg_label_lists_host (which
the CPU tier, test_labels_host.py, holds against the np_labels model), byte for byte.

  hand-built lists   tests/depth_cases.py with test_labels_host's hand-given owners at 64x40 (one strip), 131x67 (partial last strip), 5x9
                     (narrower than a wave) and 96x200 (crosses the 128-row band: a run and a box span two workgroups); a map object
                     straddles x = 63|64; sub-range readbacks, each output NULL in turn, the box rows of frame i when first > 0
  views              dg_render_label_views == the host function on dg_build_lists_owners output: 16 path frames at 320x200 and 2 at
                     1280x800 on the light map, 8 at 320x200 on the heavy map, on ctxs of every front end; with per-view states that set
                     objects to S_NULL (box -1); with wall effects and map-object thinkers on
  pipelining         a label slot and a colour slot in flight together
  slot rules         the refused calls, dg_slot_timing, label after colour and colour after label, dg_upload_scene
  plane layout       the slab behind dg_slot_framebuffer for n = 3 at 5x9
  stale rows         a second submission with fewer frames on the same slot
"""
import ctypes

import numpy as np
import pytest

import depth_cases
import mobj_fx as mf
from test_edge_kats import to_dg_lists, view_dict
from test_labels_host import hand_owners

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
MOBJ = 2


def _same(got, want, what):
    for name, g, w in (("id", got[0], want[0]), ("cls", got[1], want[1])):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} pixels differ, first at {bad[0].tolist()}: gpu {g[tuple(bad[0])]} host {w[tuple(bad[0])]}"
    bad = np.argwhere(got[2] != want[2])
    assert len(bad) == 0, f"{what}: {len(bad)} boxes differ, first at (frame, map object) {bad[0].tolist()}: gpu {got[2][tuple(bad[0])]} host {want[2][tuple(bad[0])]}"


def _host_of_views(dg, scene, W, H, views):
    """dg_label_lists_host on dg_build_lists_owners output, one view at a time (the lists live in a per-thread arena)."""
    ids = np.empty((len(views), H, W), dtype=np.uint16)
    cls = np.empty((len(views), H, W), dtype=np.uint8)
    boxes = np.empty((len(views), scene.mobj_count()), dtype=dg.LABEL_BOX_DTYPE)
    for i in range(len(views)):
        fl, owners = scene.build_lists_owners(W, H, views[i])
        ids[i], cls[i], boxes[i] = [a[0] for a in dg.label_lists_host(scene, W, H, (dg.DgFrameLists * 1)(fl), [owners])]
    return ids, cls, boxes


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


def _hand_frames(dg, campath_mod, scene, W, H, only=None):
    cs = [c for c in depth_cases.cases(W, H) if only is None or c[0] in only]
    keep, frames, owners = [], (dg.DgFrameLists * len(cs))(), []
    for i, (name, v, lists) in enumerate(cs):
        rec, _vd = view_dict(campath_mod, *v)
        frames[i], k = to_dg_lists(dg, scene, rec, lists)
        keep.append(k)
        owners.append(hand_owners(dg, lists, 1000, scene.mobj_count()))
    return frames, owners, keep


@pytest.mark.parametrize("size", [(64, 40), (131, 67), (5, 9), (96, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hand_built_lists_equal_the_host_function(dg, campath_mod, scene1993, size):
    W, H = size
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H)
    n = len(frames)
    want = dg.label_lists_host(scene1993, W, H, frames, owners)
    assert all((want[1][i] == MOBJ).any() for i in range(n))
    if W > 64:                                                       # a map object's box straddles the strip boundary x = 63|64 ...
        assert any(b["pixels"] > 0 and b["x0"] <= 63 and b["x1"] >= 64 for b in want[2].reshape(-1))
    if H > 128:                                                      # ... and one a run across the band boundary y = 127|128
        assert ((want[1][:, 127, :] == MOBJ) & (want[1][:, 128, :] == MOBJ) & (want[0][:, 127, :] == want[0][:, 128, :])).any()
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scene1993)
    op, keep_o = dg.owner_pointers(owners)
    assert dg.lib().dg_label_lists(ctx._h, 0, frames, op, n, None, None, None) == dg.DG_OK       # no output: the call only waits
    _same(ctx.readback_labels(0, 0, n), want, f"{W}x{H}")
    for k in range(3):                                               # each output alone, on a sub-range with first > 0
        flags = [i == k for i in range(3)]
        out = ctx.readback_labels(0, 1, n - 1, *flags)
        assert [o is not None for o in out] == flags and np.array_equal(out[k], want[k][1:])
    for k in range(3):                                               # each output NULL in turn, the last frame alone
        flags = [i != k for i in range(3)]
        out = ctx.readback_labels(0, n - 1, 1, *flags)
        assert all(np.array_equal(out[i], want[i][n - 1:]) for i in range(3) if i != k) and out[k] is None
    assert dg.lib().dg_readback_labels(ctx._h, 0, 2, 0, None, None, None) == dg.DG_OK            # count = 0 does nothing
    for (first, count) in ((-1, 1), (0, n + 1), (n, 1), (0, -1)):
        assert dg.lib().dg_readback_labels(ctx._h, 0, first, count, None, None, None) == dg.DG_ERR_INVALID
    _same(ctx.label_lists(0, frames, owners), want, f"{W}x{H} again")                             # the synchronous call with every output
    assert ctx.timing(0)["front_end"] == dg.DG_FE_LABELS
    ctx.close()
    del keep, keep_o


def test_refused_owner_tags_launch_nothing(dg, campath_mod, scene1993):
    W, H = 64, 40
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H)
    n = len(frames)
    want = dg.label_lists_host(scene1993, W, H, frames, owners)
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scene1993)
    ctx.label_lists(0, frames, owners)
    L = dg.lib()
    for tag in (dg.owner_tag(0, 0), dg.owner_tag(3, 1), dg.owner_tag(MOBJ, scene1993.mobj_count()), dg.owner_tag(1, 0xFFFF), 0xFFFFFFFF):
        bad = [o.copy() for o in owners]
        bad[n - 1][0] = tag
        op, keep_o = dg.owner_pointers(bad)
        assert L.dg_label_lists(ctx._h, 0, frames, op, n, None, None, None) == dg.DG_ERR_INVALID, hex(tag)
        assert f"frame {n - 1}".encode() in L.dg_last_error()
    op, keep_o = dg.owner_pointers(owners[:-1] + [None])
    assert L.dg_label_lists(ctx._h, 0, frames, op, n, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_label_lists(ctx._h, 0, frames, None, n, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_label_lists(ctx._h, 0, None, op, n, None, None, None) == dg.DG_ERR_INVALID
    _same(ctx.readback_labels(0, 0, n), want, "after the refused calls")        # the earlier submission's planes and boxes are intact
    ctx.close()
    del keep


@pytest.fixture(scope="module")
def view_batches(dg, scene1993, scene1994, path1993, path1994):
    """[(what, scene, W, H, views, host outputs)] — the host outputs computed once for the three front ends."""
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
        _same(ctx.render_labels(views), want, f"{what} front end {front_end}")
        assert ctx.timing(0)["front_end"] == dg.DG_FE_LABELS
        assert {1, 2, 3, 4} <= set(np.unique(want[1]).tolist()) and (want[2]["pixels"] > 0).any()
        assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
        ctx.close()


def test_per_view_states_that_set_objects_to_s_null(dg, wad1993, path1993):
    """Every view carries a snapshot that takes the objects the plain frame shows away (S_NULL) and gives others another sprite; the host
    outputs come from a second scene object with the same states set on the scene itself."""
    W, H = 320, 200
    idx = [0, 100, 297, 323, 500, 623, 728, 900]
    sc = dg.Scene(wad1993, "e1m1")
    handle = sc.sprite_frame("BAR1", 0)
    views = dg.make_views(path1993[idx])
    plain = _host_of_views(dg, sc, W, H, views)
    states, nulled = [], 0
    want = [np.empty_like(a) for a in plain]
    for k in range(len(idx)):
        ref = dg.Scene(wad1993, "e1m1")
        ref.sprite_frame("BAR1", 0)                                  # the same bitmap decoded in the same order: the same ids
        seen = np.nonzero(plain[2][k]["pixels"] > 0)[0].tolist()
        mobjs = []
        for j, m in enumerate(seen):
            if j % 2 == 0:
                mobjs.append((m, -1, 0))
                ref.set_mobj_state(m, None, 0, False)
                nulled += 1
            else:
                mobjs.append((m, handle, 1))
                ref.set_mobj_state(m, "BAR1", 0, True)
        states.append(([], mobjs))
        got = _host_of_views(dg, ref, W, H, views[k:k + 1])
        for a, g in zip(want, got):
            a[k] = g[0]
        for (m, frame, _fb) in mobjs:
            if frame < 0:
                assert tuple(want[2][k][m]) == (0, -1, -1, -1, -1)   # an object in S_NULL has the -1 box
        ref.close()
    assert nulled > 3 and not np.array_equal(plain[1], want[1])
    ctx = dg.Context(W, H, max_batch=len(idx), slots=1, front_end=3)
    ctx.upload_scene(sc)
    st, keep = dg.make_view_states(states)
    _same(ctx.render_labels(views, st), want, "per-view states")
    _same(ctx.render_labels(views), plain, "no states")
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
    want = _host_of_views(dg, sc, W, H, views)                       # dg_build_lists_owners draws with the scene's effects at each view's timestamp
    still = dg.make_views(path1993[idx])
    assert not np.array_equal(_host_of_views(dg, sc, W, H, still)[0], want[0])    # the timestamps show in the id plane
    ctx = dg.Context(W, H, max_batch=len(idx), slots=1, front_end=3)
    ctx.upload_scene(sc)
    _same(ctx.render_labels(views), want, "effects on")
    ctx.close()
    sc.close()


def test_a_label_slot_and_a_colour_slot_in_flight_together(dg, scene1993, view_batches):
    what, sc, W, H, views, want = view_batches[0]
    n = len(views)
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    ctx.submit(1, views)
    ctx.wait(1)
    alone = ctx.frame_checksums(1, 0, n)
    ctx.submit(1, views)
    ctx.submit_labels(0, views)
    ctx.submit(1, views)                                             # a second colour batch behind the label kernels
    ctx.wait(0)
    ctx.wait(1)
    assert np.array_equal(ctx.frame_checksums(1, 0, n), alone)
    _same(ctx.readback_labels(0, 0, n), want, "labels next to colour")
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    ctx.close()


def test_a_second_submission_with_fewer_frames(dg, scene1993, path1993, view_batches):
    """The box table keeps the first submission's rows beyond the second's frames: they are neither read nor reachable."""
    what, sc, W, H, views, want = view_batches[0]
    n = len(views)
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scene1993)
    ctx.submit_labels(0, views)
    few = dg.make_views(path1993[0:960:60][[9, 3, 12]])
    ctx.submit_labels(0, few)
    got = ctx.readback_labels(0, 0, 3)
    _same(got, [a[[9, 3, 12]] for a in want], "the second submission")
    _same(ctx.readback_labels(0, 2, 1), [a[[12]] for a in want], "its last frame alone")          # the box row of frame i when first > 0
    assert dg.lib().dg_readback_labels(ctx._h, 0, 0, 4, None, None, None) == dg.DG_ERR_INVALID
    assert dg.lib().dg_readback_labels(ctx._h, 0, 3, 1, None, None, None) == dg.DG_ERR_INVALID
    ctx.close()


def test_slot_rules(dg, scene1993, scene1994, path1993, view_batches):
    what, sc, W, H, views, want = view_batches[0]
    n = len(views)
    L = dg.lib()
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    colour = ctx.render(views)
    assert L.dg_readback_labels(ctx._h, 0, 0, 1, None, None, None) == dg.DG_ERR_INVALID          # the last submission is colour
    assert L.dg_readback_labels(ctx._h, 1, 0, 0, None, None, None) == dg.DG_ERR_INVALID          # ... or nothing at all
    assert L.dg_slot_label_timing(ctx._h, 0, None, None) == dg.DG_ERR_INVALID
    ctx.submit_depth(0, views)
    assert L.dg_readback_labels(ctx._h, 0, 0, 1, None, None, None) == dg.DG_ERR_INVALID          # ... or depth
    # a label submission on a slot with a pending dg_readback_async completes that readback first
    nbytes = n * ctx.frame_bytes
    buf = L.dg_alloc_host(nbytes)
    host = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
    host[:] = 0xA5
    ctx.submit(0, views)
    ctx.readback_async(0, 0, n, buf)
    ctx.submit_labels(0, views)
    assert np.array_equal(host.reshape(colour.shape), colour)
    _same(ctx.readback_labels(0, 0, n), want, "labels after colour")
    t = ctx.timing(0)
    assert t["front_end"] == dg.DG_FE_LABELS and t["n_frames"] == n and t["raster_ms"] > 0 and t["setup_ms"] == 0
    lt = ctx.label_timing(0)
    assert lt["tiles_ms"] > 0 and lt["boxes_ms"] > 0 and lt["tiles_ms"] + lt["boxes_ms"] <= t["raster_ms"] * 1.001 + 1e-3
    # the calls that would read the planes as RGB24 or as depth, or run the colour kernels on the slot again
    out = np.zeros(nbytes, dtype=np.uint8)
    desc = dg.DgReduceDesc(2, 2, 0, 0)
    sums = np.zeros(n, dtype=np.uint64)
    d16 = np.zeros(W * H, dtype=np.int16)
    refused = [L.dg_readback(ctx._h, 0, 0, 1, out.ctypes.data_as(P)), L.dg_readback_async(ctx._h, 0, 0, 1, P(buf)),
               L.dg_readback_reduced(ctx._h, 0, 0, 1, ctypes.byref(desc), out.ctypes.data_as(P)),
               L.dg_readback_reduced_async(ctx._h, 0, 0, 1, ctypes.byref(desc), P(buf)),
               L.dg_frame_checksums(ctx._h, 0, 0, 1, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), L.dg_replay_slot(ctx._h, 0)]
    assert refused == [dg.DG_ERR_INVALID] * 6
    assert b"label" in L.dg_last_error()
    assert L.dg_readback_depth(ctx._h, 0, 0, 1, d16.ctypes.data_as(P), None) == dg.DG_ERR_INVALID
    assert not out.any() and not sums.any() and not d16.any()
    ctx.wait(0)
    _same(ctx.readback_labels(0, 0, n), want, "after the refused calls")
    assert isinstance(ctx.framebuffer_ptr(0), int)
    # a colour submission into the slot that held labels
    ctx.submit(0, views)
    assert np.array_equal(ctx.readback(0, 0, n), colour)
    assert ctx.timing(0)["front_end"] == 2
    assert L.dg_readback_labels(ctx._h, 0, 0, 1, None, None, None) == dg.DG_ERR_INVALID
    # dg_upload_scene with a label slot in flight; another scene has another number of map objects: the box table follows
    ctx.submit_labels(1, views)
    ctx.upload_scene(scene1994)
    assert L.dg_readback_labels(ctx._h, 1, 0, 1, None, None, None) == dg.DG_ERR_INVALID          # every slot is empty after an upload
    assert scene1994.mobj_count() != scene1993.mobj_count()
    two = dg.make_views(path1993[0:120:60])
    _same(ctx.render_labels(two), _host_of_views(dg, scene1994, W, H, two), "after the upload of another scene")
    ctx.upload_scene(scene1993)
    _same(ctx.render_labels(views), want, "after the upload")
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    # errors of the submission itself
    assert L.dg_submit_label_views(ctx._h, 0, None, None, n) == dg.DG_ERR_INVALID
    assert L.dg_submit_label_views(ctx._h, 2, views, None, n) == dg.DG_ERR_INVALID
    assert L.dg_submit_label_views(ctx._h, 0, views, None, n + 1) == dg.DG_ERR_CAPACITY
    L.dg_free_host(buf)
    ctx.close()


def test_plane_layout_in_the_framebuffer_slab(dg, campath_mod, scene1993):
    """n = 3 at 5x9: uint16 id[3][9][5] at the slab's base, uint8 cls[3][9][5] at byte offset 2 * 3 * 45.  The slab's 3 * n * W * H raw
    bytes are copied, device to device, into a finished colour slot (dg_reduce_device with 1x1 boxes is a copy) and read from there."""
    W, H, n = 5, 9, 3
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H, only=("horizon", "wall_corners", "masked_over_floor"))
    assert len(frames) == n
    want = dg.label_lists_host(scene1993, W, H, frames, owners)
    ctx = dg.Context(W, H, max_batch=n, slots=2)
    ctx.upload_scene(scene1993)
    ctx.draw_lists(1, frames)                                        # slot 1: a finished colour submission of n frames
    ctx.label_lists(0, frames, owners)
    ctx.reduce_device(ctx.framebuffer_ptr(0), W, H, n, (1, 1), ctx.framebuffer_ptr(1))
    raw = ctx.readback(1, 0, n).reshape(-1)
    assert raw.size == 3 * n * W * H
    assert np.array_equal(raw[:2 * n * W * H].view("<u2").reshape(n, H, W), want[0])
    assert np.array_equal(raw[2 * n * W * H:].reshape(n, H, W), want[1])
    assert (want[0] != 0).any()
    ctx.close()
    del keep
