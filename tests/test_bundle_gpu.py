"""GPU tier of the bundle submission: one list build, the colour kernels and dg_bundle_tiles through the ctx entry points, every part byte for
byte against what its own route gives — colour against dg_draw_lists / dg_render_views_state on a DG_FE_HOST ctx, the depth planes against
dg_depth_lists_host, the label planes and boxes against dg_label_lists_host (test_bundle_host.py holds dg_bundle_lists_host equal to those).

  hand-built lists   tests/depth_cases.py with test_labels_host's hand-given owners through dg_bundle_lists, all three parts, at 64x40 (one
                     strip), 131x67 (partial last strip), 5x9 (narrower than a wave) and 96x200 (crosses the 128-row band; a box straddles
                     x = 63|64); sub-range readbacks, each output NULL in turn
  every `what`       the seven masks at 131x67: the requested parts, DG_ERR_INVALID for the others, dg_slot_timing and dg_slot_bundle_timing
  views              dg_submit_bundle_views: 16 path frames at 320x200 and 2 at 1280x800 on the light map, 8 at 320x200 on the heavy map, on
                     ctxs of every front end; with per-view states (S_NULL, other sprite frames); with wall effects, light effects and
                     map-object thinkers on
  slot rules         pipelining next to a colour slot, slot reuse in every order, stale rows, dg_upload_scene of a scene with another number
                     of map objects, the capacity, refused tags, dg_replay_slot, the reduced readback, the slab's layout
"""
import ctypes

import numpy as np
import pytest

import depth_cases
import mobj_fx as mf
from staging_cases import bundle_batch_for as _batch_for
from test_edge_kats import to_dg_lists, view_dict
from test_labels_host import hand_owners

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
MOBJ = 2
ALL = 7
DEPTH_NAMES, LABEL_NAMES = ("distance", "kind"), ("id", "cls", "boxes")


def _same(names, got, want, what):
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} entries differ, first at {bad[0].tolist()}: gpu {g[tuple(bad[0])]} host {w[tuple(bad[0])]}"


def _same_colour(got, want, what):
    bad = np.argwhere(np.any(got != want, axis=3))
    assert len(bad) == 0, f"{what}: {len(bad)} colour pixels differ, first at (frame, y, x) {bad[0].tolist()}: bundle {got[tuple(bad[0])]} colour route {want[tuple(bad[0])]}"


def _capacity(dg, W, H, max_batch, what):
    """dg_bundle_capacity's rule restated on dg_bundle_layout (test_bundle_host.py holds that against the stated layout)."""
    return max([n for n in range(1, max_batch + 1) if dg.bundle_layout(W, H, n, what)["total"] <= max_batch * 3 * W * H], default=0)


def _check_parts(dg, ctx, slot, n, what, colour, depth, labels, tag):
    """Every part of the slot's bundle against the expected arrays (those of the parts asked for), the others refused."""
    L = dg.lib()
    if what & dg.DG_BUNDLE_COLOUR:
        _same_colour(ctx.readback(slot, 0, n), colour, tag)
    else:
        out = np.zeros(ctx.frame_bytes, dtype=np.uint8)
        sums = np.zeros(1, dtype=np.uint64)
        assert L.dg_readback(ctx._h, slot, 0, 1, out.ctypes.data_as(P)) == dg.DG_ERR_INVALID and b"colour" in L.dg_last_error()
        assert L.dg_frame_checksums(ctx._h, slot, 0, 1, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == dg.DG_ERR_INVALID
        assert not out.any() and not sums.any()
    if what & dg.DG_BUNDLE_DEPTH:
        _same(DEPTH_NAMES, ctx.readback_depth(slot, 0, n), depth, tag)
    else:
        assert L.dg_readback_depth(ctx._h, slot, 0, 1, None, None) == dg.DG_ERR_INVALID and b"depth" in L.dg_last_error()
    if what & dg.DG_BUNDLE_LABELS:
        _same(LABEL_NAMES, ctx.readback_labels(slot, 0, n), labels, tag)
    else:
        assert L.dg_readback_labels(ctx._h, slot, 0, 1, None, None, None) == dg.DG_ERR_INVALID and b"label" in L.dg_last_error()


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


def _host_of_lists(dg, scene, W, H, frames, owners):
    return dg.depth_lists_host(scene, W, H, frames), dg.label_lists_host(scene, W, H, frames, owners)


def _host_of_views(dg, scene, W, H, views):
    """dg_depth_lists_host and dg_label_lists_host on dg_build_lists_owners output, one view at a time (the lists live in a per-thread arena)."""
    n = len(views)
    d, k = np.empty((n, H, W), dtype=np.int16), np.empty((n, H, W), dtype=np.uint8)
    ids, cls = np.empty((n, H, W), dtype=np.uint16), np.empty((n, H, W), dtype=np.uint8)
    boxes = np.empty((n, scene.mobj_count()), dtype=dg.LABEL_BOX_DTYPE)
    for i in range(n):
        fl, owners = scene.build_lists_owners(W, H, views[i])
        frames = (dg.DgFrameLists * 1)(fl)
        d[i], k[i] = [a[0] for a in dg.depth_lists_host(scene, W, H, frames)]
        ids[i], cls[i], boxes[i] = [a[0] for a in dg.label_lists_host(scene, W, H, frames, [owners])]
    return (d, k), (ids, cls, boxes)


def _colour_of_views(dg, scene, W, H, views, states=None):
    """dg_render_views_state of the views on a DG_FE_HOST ctx of their own size."""
    ctx = dg.Context(W, H, max_batch=len(views), slots=1, front_end=dg.DG_FE_HOST)
    ctx.upload_scene(scene)
    out = ctx.render_state(views, states)
    ctx.close()
    return out


# ---- hand-built lists ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(64, 40), (131, 67), (5, 9), (96, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hand_built_lists_all_three_parts(dg, campath_mod, scene1993, size):
    W, H = size
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H)
    n = len(frames)
    depth, labels = _host_of_lists(dg, scene1993, W, H, frames, owners)
    assert all((labels[1][i] == MOBJ).any() for i in range(n))
    if W > 64:                                                       # a map object's box straddles the strip boundary x = 63|64 ...
        assert any(b["pixels"] > 0 and b["x0"] <= 63 and b["x1"] >= 64 for b in labels[2].reshape(-1))
    if H > 128:                                                      # ... and a run of one id crosses the band boundary y = 127|128
        assert ((labels[1][:, 127, :] == MOBJ) & (labels[1][:, 128, :] == MOBJ) & (labels[0][:, 127, :] == labels[0][:, 128, :])).any()
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=2)
    ctx.upload_scene(scene1993)
    assert ctx.bundle_capacity(ALL) >= n
    colour = ctx.draw_lists(1, frames)                               # the colour route, on a second slot of the same ctx
    ctx.bundle_lists(0, frames, owners, ALL)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, f"{W}x{H}")
    assert np.array_equal(ctx.frame_checksums(0, 0, n), ctx.frame_checksums(1, 0, n))
    # sub-ranges with first > 0; each output alone and each output NULL in turn
    assert np.array_equal(ctx.readback(0, 1, n - 1), colour[1:])
    for k in range(2):
        flags = [i == k for i in range(2)]
        out = ctx.readback_depth(0, 1, n - 1, *flags)
        assert [o is not None for o in out] == flags and np.array_equal(out[k], depth[k][1:])
    for k in range(3):
        flags = [i == k for i in range(3)]
        out = ctx.readback_labels(0, 1, n - 1, *flags)
        assert [o is not None for o in out] == flags and np.array_equal(out[k], labels[k][1:])
        flags = [i != k for i in range(3)]
        out = ctx.readback_labels(0, n - 1, 1, *flags)
        assert all(np.array_equal(out[i], labels[i][n - 1:]) for i in range(3) if i != k) and out[k] is None
    L = dg.lib()
    assert L.dg_readback_depth(ctx._h, 0, 2, 0, None, None) == dg.DG_OK and L.dg_readback_labels(ctx._h, 0, 2, 0, None, None, None) == dg.DG_OK
    for (first, count) in ((-1, 1), (0, n + 1), (n, 1), (0, -1)):
        assert L.dg_readback_depth(ctx._h, 0, first, count, None, None) == dg.DG_ERR_INVALID
        assert L.dg_readback_labels(ctx._h, 0, first, count, None, None, None) == dg.DG_ERR_INVALID
    t = ctx.timing(0)
    assert t["front_end"] == dg.DG_FE_BUNDLE and t["n_frames"] == n
    ctx.close()
    del keep


@pytest.mark.parametrize("what", range(1, 8))
def test_each_what_at_131x67(dg, campath_mod, scene1993, what):
    W, H = 131, 67
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H)
    n = len(frames)
    depth, labels = _host_of_lists(dg, scene1993, W, H, frames, owners)
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n, what), slots=2)
    ctx.upload_scene(scene1993)
    colour = ctx.draw_lists(1, frames)
    ctx.bundle_lists(0, frames, owners if what & dg.DG_BUNDLE_LABELS else None, what)
    _check_parts(dg, ctx, 0, n, what, colour, depth, labels, f"what {what}")
    t, bt = ctx.timing(0), ctx.bundle_timing(0)
    assert t["front_end"] == dg.DG_FE_BUNDLE and t["n_frames"] == n and t["total_ms"] > 0
    if what & dg.DG_BUNDLE_COLOUR:
        assert t["setup_ms"] > 0 and t["raster_ms"] > 0 and bt["setup_ms"] == t["setup_ms"] and bt["raster_ms"] == t["raster_ms"]
    else:
        assert t["setup_ms"] == 0 and t["raster_ms"] == 0 and bt["setup_ms"] == 0 and bt["raster_ms"] == 0
    assert (bt["tiles_ms"] > 0) == (what != dg.DG_BUNDLE_COLOUR)
    assert dg.lib().dg_slot_bundle_timing(ctx._h, 1, None, None, None) == dg.DG_ERR_INVALID      # slot 1 holds a colour submission
    assert dg.lib().dg_slot_label_timing(ctx._h, 0, None, None) == dg.DG_ERR_INVALID
    ctx.close()
    del keep


# ---- views -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def view_batches(dg, scene1993, scene1994, path1993, path1994):
    """[(what, scene, W, H, views, colour, depth, labels)] — the expected parts computed once for the three front ends."""
    out = []
    for what, sc, W, H, recs in (("light 320x200", scene1993, 320, 200, path1993[0:960:60]), ("light 1280x800", scene1993, 1280, 800, path1993[[297, 728]]),
                                 ("heavy 320x200", scene1994, 320, 200, path1994[0:1000:125])):
        views = dg.make_views(recs)
        depth, labels = _host_of_views(dg, sc, W, H, views)
        out.append((what, sc, W, H, views, _colour_of_views(dg, sc, W, H, views), depth, labels))
    assert [len(b[4]) for b in out] == [16, 2, 8]
    return out


@pytest.mark.parametrize("front_end", [1, 2, 3], ids=["host-lists", "device-column-walk", "device-seg-walk"])
def test_views_whatever_the_front_end(dg, view_batches, front_end):
    for what, sc, W, H, views, colour, depth, labels in view_batches:
        n = len(views)
        ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=1, front_end=front_end)
        ctx.upload_scene(sc)
        ctx.submit_bundle(0, views, ALL)
        _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, f"{what} front end {front_end}")
        assert ctx.timing(0)["front_end"] == dg.DG_FE_BUNDLE         # always the host list route, and the ctx says so
        got = ctx.readback(0, 0, n)
        assert ctx.frame_checksums(0, 0, n).tolist() == [dg.frame_checksum(got[i]) for i in range(n)]
        assert {1, 2, 3, 4} <= set(np.unique(labels[1]).tolist()) and (labels[2]["pixels"] > 0).any() and {1, 2, 3} <= set(np.unique(depth[1]).tolist())
        assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
        ctx.close()


def test_per_view_states_that_set_objects_to_s_null(dg, wad1993, path1993):
    """Every view carries a snapshot that takes the objects the plain frame shows away (S_NULL) and gives others another sprite; the
    expected planes come from a second scene object with the same states set on the scene itself, the colour from the colour route."""
    W, H = 320, 200
    idx = [0, 100, 297, 323, 500, 623, 728, 900]
    n = len(idx)
    sc = dg.Scene(wad1993, "e1m1")
    handle = sc.sprite_frame("BAR1", 0)
    views = dg.make_views(path1993[idx])
    plain_depth, plain_labels = _host_of_views(dg, sc, W, H, views)
    states, nulled = [], 0
    depth = [np.empty_like(a) for a in plain_depth]
    labels = [np.empty_like(a) for a in plain_labels]
    for k in range(n):
        ref = dg.Scene(wad1993, "e1m1")
        ref.sprite_frame("BAR1", 0)                                  # the same bitmap decoded in the same order: the same ids
        seen = np.nonzero(plain_labels[2][k]["pixels"] > 0)[0].tolist()
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
        d, l = _host_of_views(dg, ref, W, H, views[k:k + 1])
        for a, g in zip(depth + labels, d + l):
            a[k] = g[0]
        for (m, frame, _fb) in mobjs:
            if frame < 0:
                assert tuple(labels[2][k][m]) == (0, -1, -1, -1, -1)   # an object in S_NULL has the -1 box
        ref.close()
    assert nulled > 3 and not np.array_equal(plain_labels[1], labels[1]) and not np.array_equal(plain_depth[0], depth[0])
    st, keep = dg.make_view_states(states)
    colour = _colour_of_views(dg, sc, W, H, views, st)
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=1, front_end=3)
    ctx.upload_scene(sc)
    ctx.submit_bundle(0, views, ALL, states=st)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "per-view states")
    ctx.submit_bundle(0, views, dg.DG_BUNDLE_DEPTH | dg.DG_BUNDLE_LABELS)
    _check_parts(dg, ctx, 0, n, 6, None, plain_depth, plain_labels, "no states")
    ctx.close()
    sc.close()
    del keep


def test_wall_effects_light_effects_and_map_object_thinkers_on(dg, path1993):
    W, H = 320, 200
    sc = dg.Scene(mf.fx_wad(), "E1M1")
    sc.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
    sc.set_light_effects(dg.DG_LIGHT_THINKERS, 1993)
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    sc.mobj_event(dg.DG_MOBJ_KILL, mf.ts(140))
    idx = [0, 54, 140, 266, 404, 541, 703, 879]
    n = len(idx)
    views = dg.make_views(path1993[idx])
    for k, T in enumerate((1, 7, 139, 141, 148, 160, 200, 300)):
        views[k].timestamp = mf.ts(T)
    depth, labels = _host_of_views(dg, sc, W, H, views)              # dg_build_lists_owners draws with the scene's effects at each view's timestamp
    still = dg.make_views(path1993[idx])
    assert not np.array_equal(_host_of_views(dg, sc, W, H, still)[1][0], labels[0])     # the timestamps show in the id plane
    colour = _colour_of_views(dg, sc, W, H, views)
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=1, front_end=3)
    ctx.upload_scene(sc)
    ctx.submit_bundle(0, views, ALL)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "effects on")
    ctx.close()
    sc.close()


# ---- slot rules and state --------------------------------------------------------------------------------------------------------------------

def test_a_bundle_slot_and_a_colour_slot_in_flight_together(dg, scene1993, view_batches):
    what, sc, W, H, views, colour, depth, labels = view_batches[0]
    n = len(views)
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    ctx.submit(1, views)
    ctx.wait(1)
    alone = ctx.frame_checksums(1, 0, n)
    ctx.submit(1, views)
    ctx.submit_bundle(0, views, ALL)
    ctx.submit(1, views)                                             # a second colour batch behind the bundle's kernels
    ctx.wait(0)
    ctx.wait(1)
    assert np.array_equal(ctx.frame_checksums(1, 0, n), alone)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "bundle next to colour")
    assert np.array_equal(ctx.frame_checksums(0, 0, n), alone)
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    ctx.close()


def test_slot_reuse_stale_rows_scene_change_replay_and_reduced_readback(dg, scene1993, scene1994, path1993, view_batches):
    what, sc, W, H, views, colour, depth, labels = view_batches[0]
    n = len(views)
    L = dg.lib()
    ctx = dg.Context(W, H, max_batch=_batch_for(dg, W, H, n), slots=2, front_end=2)
    ctx.upload_scene(scene1993)
    assert L.dg_slot_bundle_timing(ctx._h, 0, None, None, None) == dg.DG_ERR_INVALID             # nothing at all on the slot
    # a bundle after a colour, a depth and a label submission on one slot, and each of those after a bundle
    ctx.submit(0, views)
    ctx.submit_bundle(0, views, ALL)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "bundle after colour")
    ctx.submit_depth(0, views)
    _same(DEPTH_NAMES, ctx.readback_depth(0, 0, n), depth, "depth after bundle")
    assert L.dg_readback_labels(ctx._h, 0, 0, 1, None, None, None) == dg.DG_ERR_INVALID
    ctx.submit_bundle(0, views, ALL)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "bundle after depth")
    ctx.submit_labels(0, views)
    _same(LABEL_NAMES, ctx.readback_labels(0, 0, n), labels, "labels after bundle")
    assert L.dg_readback_depth(ctx._h, 0, 0, 1, None, None) == dg.DG_ERR_INVALID
    ctx.submit_bundle(0, views, ALL)
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "bundle after labels")
    # the reduced readback of the colour part, and the calls a bundle slot refuses
    full = ctx.readback(0, 0, n)
    assert np.array_equal(ctx.readback_reduced(0, 0, n, (2, 2)), dg.reduce_host(full, (2, 2)))
    assert np.array_equal(ctx.readback_reduced(0, 3, 2, (4, 3, dg.DG_REDUCE_GRAY8)), dg.reduce_host(full[3:5], (4, 3, dg.DG_REDUCE_GRAY8)))
    assert L.dg_replay_slot(ctx._h, 0) == dg.DG_ERR_INVALID and b"bundle" in L.dg_last_error()
    _check_parts(dg, ctx, 0, n, ALL, colour, depth, labels, "after the refused replay")
    ctx.submit(0, views)
    _same_colour(ctx.readback(0, 0, n), colour, "colour after bundle")
    assert ctx.timing(0)["front_end"] == 2
    assert L.dg_readback_depth(ctx._h, 0, 0, 1, None, None) == dg.DG_ERR_INVALID and L.dg_slot_bundle_timing(ctx._h, 0, None, None, None) == dg.DG_ERR_INVALID
    # stale rows: a second bundle with fewer frames and another `what` on the same slot
    ctx.submit_bundle(0, views, ALL)
    pick = [9, 3, 12]
    few = dg.make_views(path1993[0:960:60][pick])
    ctx.submit_bundle(0, few, dg.DG_BUNDLE_LABELS)
    _check_parts(dg, ctx, 0, 3, dg.DG_BUNDLE_LABELS, None, None, [a[pick] for a in labels], "the second bundle")
    _same(LABEL_NAMES, ctx.readback_labels(0, 2, 1), [a[[12]] for a in labels], "its last frame alone")
    assert L.dg_readback_labels(ctx._h, 0, 0, 4, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_readback_labels(ctx._h, 0, 3, 1, None, None, None) == dg.DG_ERR_INVALID
    ctx.submit_bundle(0, few, dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH)
    _check_parts(dg, ctx, 0, 3, 3, colour[pick], [a[pick] for a in depth], None, "the third bundle")
    # dg_upload_scene with a bundle in flight; the other scene has another number of map objects: the box table follows
    ctx.submit_bundle(1, views, ALL)
    ctx.upload_scene(scene1994)
    assert L.dg_readback_labels(ctx._h, 1, 0, 1, None, None, None) == dg.DG_ERR_INVALID          # every slot is empty after an upload
    assert L.dg_readback(ctx._h, 1, 0, 1, None) == dg.DG_ERR_INVALID
    assert scene1994.mobj_count() != scene1993.mobj_count()
    two = dg.make_views(path1993[0:120:60])
    d2, l2 = _host_of_views(dg, scene1994, W, H, two)
    ctx.submit_bundle(1, two, ALL)
    _check_parts(dg, ctx, 1, 2, ALL, _colour_of_views(dg, scene1994, W, H, two), d2, l2, "after the upload of another scene")
    ctx.upload_scene(scene1993)
    ctx.submit_bundle(1, views, ALL)
    _check_parts(dg, ctx, 1, n, ALL, colour, depth, labels, "after the upload")
    assert ctx.fallbacks() == {"front_end": 0, "redone_frames": 0}
    # errors of the submission itself
    assert L.dg_submit_bundle_views(ctx._h, 0, None, None, n, ALL) == dg.DG_ERR_INVALID
    assert L.dg_submit_bundle_views(ctx._h, 2, views, None, n, ALL) == dg.DG_ERR_INVALID
    for bad in (0, 8, 0xFFFFFFFF):
        assert L.dg_submit_bundle_views(ctx._h, 0, views, None, n, bad) == dg.DG_ERR_INVALID
        assert L.dg_bundle_capacity(ctx._h, bad) == dg.DG_ERR_INVALID
    assert L.dg_bundle_capacity(None, ALL) == dg.DG_ERR_INVALID
    ctx.close()


def test_the_capacity_and_refused_tags(dg, campath_mod, scene1993):
    W, H, max_batch = 64, 40, 16
    frames5, owners5, keep = _hand_frames(dg, campath_mod, scene1993, W, H)
    ctx = dg.Context(W, H, max_batch=max_batch, slots=1)
    ctx.upload_scene(scene1993)
    for what in range(1, 8):
        assert ctx.bundle_capacity(what) == _capacity(dg, W, H, max_batch, what), what
    cap = ctx.bundle_capacity(ALL)
    assert cap == 5 == len(frames5) and ctx.bundle_capacity(dg.DG_BUNDLE_COLOUR) == max_batch
    depth, labels = _host_of_lists(dg, scene1993, W, H, frames5, owners5)
    ctx.bundle_lists(0, frames5, owners5, ALL)                       # n = capacity works
    _same(DEPTH_NAMES, ctx.readback_depth(0, 0, cap), depth, "n = capacity")
    _same(LABEL_NAMES, ctx.readback_labels(0, 0, cap), labels, "n = capacity")
    colour = ctx.readback(0, 0, cap)
    L = dg.lib()
    frames6 = (dg.DgFrameLists * 6)(*[frames5[i % 5] for i in range(6)])
    op6, keep6 = dg.owner_pointers([owners5[i % 5] for i in range(6)])
    assert L.dg_bundle_lists(ctx._h, 0, frames6, op6, 6, ALL) == dg.DG_ERR_CAPACITY              # n = capacity + 1 <= max_batch
    assert b"dg_bundle_capacity" in L.dg_last_error()
    assert ctx.bundle_capacity(3) == 8 and L.dg_bundle_lists(ctx._h, 0, frames6, op6, 6, dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH) == dg.DG_OK    # (six fit without the labels)
    ctx.bundle_lists(0, frames5, owners5, ALL)
    # refused tags launch nothing and leave the earlier content readable
    for tag in (dg.owner_tag(0, 0), dg.owner_tag(3, 1), dg.owner_tag(MOBJ, scene1993.mobj_count()), dg.owner_tag(1, 0xFFFF), 0xFFFFFFFF):
        bad = [o.copy() for o in owners5]
        bad[4][0] = tag
        op, keep_o = dg.owner_pointers(bad)
        assert L.dg_bundle_lists(ctx._h, 0, frames5, op, 5, ALL) == dg.DG_ERR_INVALID, hex(tag)
        assert b"frame 4" in L.dg_last_error()
    op, keep_o = dg.owner_pointers(owners5[:-1] + [None])
    assert L.dg_bundle_lists(ctx._h, 0, frames5, op, 5, ALL) == dg.DG_ERR_INVALID
    assert L.dg_bundle_lists(ctx._h, 0, frames5, None, 5, dg.DG_BUNDLE_LABELS) == dg.DG_ERR_INVALID
    assert L.dg_bundle_lists(ctx._h, 0, None, op, 5, ALL) == dg.DG_ERR_INVALID
    assert L.dg_bundle_lists(ctx._h, 0, frames6, op6, 6, ALL) == dg.DG_ERR_CAPACITY
    _check_parts(dg, ctx, 0, cap, ALL, colour, depth, labels, "after the refused calls")
    assert ctx.timing(0)["n_frames"] == cap
    ctx.close()
    # a ctx whose slab does not hold even one frame of all three parts
    small = dg.Context(5, 9, max_batch=3, slots=1)
    small.upload_scene(scene1993)
    assert small.bundle_capacity(ALL) == 0 and small.bundle_capacity(dg.DG_BUNDLE_COLOUR) == 3
    f1, o1, k1 = _hand_frames(dg, campath_mod, scene1993, 5, 9, only=("horizon",))
    op1, keep1 = dg.owner_pointers(o1)
    assert L.dg_bundle_lists(small._h, 0, f1, op1, 1, ALL) == dg.DG_ERR_CAPACITY
    assert L.dg_bundle_lists(small._h, 0, f1, None, 1, dg.DG_BUNDLE_COLOUR) == dg.DG_OK
    small.close()
    del keep, keep6, keep_o, k1, keep1


def test_the_slab_matches_the_layout(dg, campath_mod, scene1993):
    """n = 3 at 5x9, all three parts: the slab behind dg_slot_framebuffer holds each part at dg_bundle_layout's offset.  The slab's raw
    bytes are copied, device to device, into a finished colour slot (dg_reduce_device with 1x1 boxes is a copy) and read from there."""
    W, H, n = 5, 9, 3
    frames, owners, keep = _hand_frames(dg, campath_mod, scene1993, W, H, only=("horizon", "wall_corners", "masked_over_floor"))
    assert len(frames) == n
    depth, labels = _host_of_lists(dg, scene1993, W, H, frames, owners)
    lay = dg.bundle_layout(W, H, n, ALL)
    mb = _batch_for(dg, W, H, n)
    assert mb == 15 and lay["total"] == 1927
    ctx = dg.Context(W, H, max_batch=mb, slots=2)
    ctx.upload_scene(scene1993)
    colour = ctx.draw_lists(1, (dg.DgFrameLists * mb)(*[frames[i % n] for i in range(mb)]))      # slot 1: a finished colour submission of mb frames
    ctx.bundle_lists(0, frames, owners, ALL)
    ctx.reduce_device(ctx.framebuffer_ptr(0), W, H, mb, (1, 1), ctx.framebuffer_ptr(1))
    raw = ctx.readback(1, 0, mb).reshape(-1)
    px = n * W * H
    assert raw.size == mb * 3 * W * H >= lay["total"]
    assert np.array_equal(raw[lay["colour"]:lay["colour"] + 3 * px].reshape(n, H, W, 3), colour[:n])
    assert np.array_equal(raw[lay["distance"]:lay["distance"] + 2 * px].view("<i2").reshape(n, H, W), depth[0])
    assert np.array_equal(raw[lay["kind"]:lay["kind"] + px].reshape(n, H, W), depth[1])
    assert np.array_equal(raw[lay["id"]:lay["id"] + 2 * px].view("<u2").reshape(n, H, W), labels[0])
    assert np.array_equal(raw[lay["cls"]:lay["cls"] + px].reshape(n, H, W), labels[1])
    assert (labels[0] != 0).any() and (depth[1] != 0).any() and colour.any()
    ctx.close()
    del keep
