"""GPU tier for the launch shapes of the plane walk (csrc/plane_kernels.hip: dg_depth_tiles / dg_label_tiles / dg_bundle_tiles, and
dg_label_boxes) and for skies with transparent texels.

  launch shapes    the grid of every tile kernel is ceil(W/64) x ceil(H/128) x n and dg_label_boxes walks 32-row pieces: one frame size per
                   decision (SIZES).  At each, the tests/depth_cases.py cases plus staging_cases.ladder and box_edges go through
                   dg_depth_lists, dg_label_lists and dg_bundle_lists (depth + labels: the nine-word span and the fused boxes; labels
                   alone) as one batch, forwards and in reversed order, and are compared with the numpy models (np_depth, np_labels)
                   directly and with the host entries.  Before every compared submission another batch goes through the same slot by the
                   same route — a wall owned by a map object over the whole frame: kind, distance, class and id all differ from what an
                   uncovered pixel holds — so a row or pixel a kernel fails to write cannot pass on stale content.
  holey skies      sky_cases.sky_lists through dg_draw_lists, dg_depth_lists and dg_label_lists for the hand WAD variants at 64x40, 131x67
                   and 65x129 against the models; the two small variants are refused by the binner (DG_ERR_RENDER) and the slot stays
                   usable.  16 path views at 320x200 and 2 at 1283x97 of the synthetic map with holey SKY1 patches through front ends 1, 2
                   and 3: colour == oracle frames, depth and labels == the host entries, dg_ctx_fallbacks stays at zero.
"""
import numpy as np
import pytest

import depth_cases
import np_depth
import np_front_end as nf
import np_labels as nl
import np_mappers as nm
import sky_cases as sk
import staging_cases as sc
from test_edge_kats import to_dg_lists, view_dict, wall
from test_labels_host import hand_owners

pytestmark = pytest.mark.gpu

SIZES = [(1, 1),            # smallest frame
         (63, 31),          # one column short of a strip, one row short of a box piece
         (64, 32),          # exactly one strip, exactly one box piece
         (65, 33),          # one column past a strip, one row past a box piece
         (64, 127),         # one row short of a band
         (65, 128),         # full last band
         (129, 129),        # last band of one row, third strip of one column
         (70, 161),         # box piece boundary 159/160/161 in the second band
         (130, 257),        # three bands
         (2, 16384)]        # tallest frame
ZERO = {"front_end": 0, "redone_frames": 0}


def _diff(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]} expected {want[tuple(bad[0])]}"


def models(names, W, H, fl, owners, n_mobjs):
    """-> (distance, kind, id, cls, boxes) of one frame from np_depth / np_labels."""
    dist, kind, _tr = np_depth.depth_of_frame_lists(names, "SKY1", W, H, fl)
    ids, cls, boxes, _tr, kind2 = nl.labels_of_frame_lists(names, "SKY1", W, H, fl, owners, n_mobjs)
    assert np.array_equal(kind, kind2)
    return dist, kind, ids, cls, boxes


@pytest.fixture(scope="module")
def world(dg, wad1993):
    scene = dg.Scene(wad1993, "e1m1")
    yield scene, np_depth.SceneNames(dg, scene, wad1993, nf), len(nf.Map(wad1993, "e1m1").segs)
    scene.close()


def cases_at(W, H):
    """depth_cases.cases(W, H) wherever its builders work: dense_strip (test_dense_columns.many_records) takes remainders by H // 2,
    a ZeroDivisionError in a frame one row high, so there ladder and box_edges go alone."""
    return [] if H < 2 else depth_cases.cases(W, H)


def shape_batch(dg, campath_mod, scene, n_segs, W, H):
    """-> (names, frames, owners, keep): the depth_cases cases, then ladder and box_edges."""
    n_mobjs = scene.mobj_count()
    cs = [(name, v, lists, hand_owners(dg, lists, n_segs, n_mobjs)) for (name, v, lists) in cases_at(W, H)]
    lad = sc.ladder(W, H)
    cs.append(("ladder", sc.LADDER_VIEW, lad, hand_owners(dg, lad, n_segs, n_mobjs)))
    lists, owners, _role = sc.box_edges(W, H, n_mobjs, n_segs)
    cs.append(("box_edges", sc.BOX_VIEW, lists, owners))
    frames, keep = (dg.DgFrameLists * len(cs))(), []
    for i, (_n, v, lists, _o) in enumerate(cs):
        rec, _vd = view_dict(campath_mod, *v)
        frames[i], k = to_dg_lists(dg, scene, rec, lists)
        keep.append(k)
    return [c[0] for c in cs], frames, [c[3] for c in cs], keep


def other_batch(dg, campath_mod, scene, W, H, n):
    """n frames of one opaque wall over the whole frame, owned by map object mobj_count - 2."""
    columns = []
    lists = {"renders": [wall("BRICK2", 144, (33.0, -70.0, 47.0, 66.0), 0, W - 1, -41.0, 87.0, [(x, 0, H - 1, H, -1) for x in range(W)], columns)],
             "columns": columns, "visplanes": [], "order": [(0, 0)]}
    rec, _vd = view_dict(campath_mod, 7.0, -3.0, 0.3, 0.0)
    fl, keep = to_dg_lists(dg, scene, rec, lists)
    owners = np.array([dg.owner_tag(nl.MOBJ, scene.mobj_count() - 2)], dtype=np.uint32)
    return (dg.DgFrameLists * n)(*([fl] * n)), [owners] * n, keep


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_shape_equals_the_models(dg, campath_mod, world, size):
    scene, names, n_segs = world
    W, H = size
    case_names, frames, owners, keep = shape_batch(dg, campath_mod, scene, n_segs, W, H)
    n = len(frames)
    assert case_names[-2:] == ["ladder", "box_edges"] and n == (2 if H < 2 else 7 if W >= 24 else 6)
    host = list(dg.depth_lists_host(scene, W, H, frames)) + list(dg.label_lists_host(scene, W, H, frames, owners))
    model = [models(names, W, H, frames[i], owners[i], scene.mobj_count()) for i in range(n)]
    model = [np.stack([m[j] for m in model]) for j in range(5)]
    other, other_owners, keep2 = other_batch(dg, campath_mod, scene, W, H, n)
    stale = list(dg.depth_lists_host(scene, W, H, other)) + list(dg.label_lists_host(scene, W, H, other, other_owners))
    # the other batch differs from what an uncovered pixel holds (far, kind 0, id 0, class 0) in every plane, everywhere
    assert (stale[0] != 32767).all() and (stale[1] == 1).all() and (stale[2] == scene.mobj_count() - 2).all() and (stale[3] == nl.MOBJ).all()
    both = dg.DG_BUNDLE_DEPTH | dg.DG_BUNDLE_LABELS
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(scene)
    bctx = dg.Context(W, H, max_batch=sc.bundle_batch_for(dg, W, H, n, both), slots=1)       # (a slab that holds the bundle's parts)
    bctx.upload_scene(scene)
    for order in (list(range(n)), list(range(n))[::-1]):
        fr = (dg.DgFrameLists * n)(*[frames[i] for i in order])
        ow = [owners[i] for i in order]
        what = f"{W}x{H} {'forwards' if order[0] == 0 else 'reversed'}"
        for g, w in zip(ctx.depth_lists(0, other), stale[:2]):
            _diff(g, w, f"{what}: the other batch, depth")
        got = ctx.depth_lists(0, fr)
        for j, plane in enumerate(("distance", "kind")):
            _diff(got[j], model[j][order], f"{what} {plane} against the model (frames {[case_names[i] for i in order]})")
            _diff(got[j], host[j][order], f"{what} {plane} against the host entry")
        for g, w in zip(ctx.label_lists(0, other, other_owners), stale[2:]):
            _diff(g, w, f"{what}: the other batch, labels")
        got = ctx.label_lists(0, fr, ow)
        for j, plane in enumerate(("id", "cls", "boxes")):
            _diff(got[j], model[2 + j][order], f"{what} {plane} against the model (frames {[case_names[i] for i in order]})")
            _diff(got[j], host[2 + j][order], f"{what} {plane} against the host entry")
        for parts, first in ((both, 0), (dg.DG_BUNDLE_LABELS, 2)):       # the bundle route: every plane of the slab dirty, then the batch
            bctx.bundle_lists(0, other, other_owners, both)
            for g, w in zip(tuple(bctx.readback_depth(0, 0, n)) + tuple(bctx.readback_labels(0, 0, n)), stale):
                _diff(g, w, f"{what}: the other batch as a bundle")
            bctx.bundle_lists(0, fr, ow, parts)
            got = (tuple(bctx.readback_depth(0, 0, n)) if first == 0 else (None, None)) + tuple(bctx.readback_labels(0, 0, n))
            for j, plane in list(enumerate(("distance", "kind", "id", "cls", "boxes")))[first:]:
                _diff(got[j], model[j][order], f"{what} bundle {parts} {plane} against the model (frames {[case_names[i] for i in order]})")
                _diff(got[j], host[j][order], f"{what} bundle {parts} {plane} against the host entry")
    assert ctx.fallbacks() == ZERO and bctx.fallbacks() == ZERO
    ctx.close()
    bctx.close()
    del keep, keep2


# ---- skies with holes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sk.VARIANTS)
def test_sky_lists_on_the_hand_wad_variants(dg, campath_mod, variant):
    wad = sk.variant_wad(variant)
    scene = dg.Scene(wad, "e1m1")
    n_segs = len(nf.Map(wad, "e1m1").segs)
    for (W, H) in ((64, 40), (131, 67), (65, 129)):
        lists = sk.sky_lists(W, H)
        ladder = sc.ladder(W, H, sc.HAND)                            # the ladder on this WAD's textures: sky spans past the staging limit
        rec, vd = view_dict(campath_mod, *sk.SKY_VIEW)
        rec2, vd2 = view_dict(campath_mod, *sc.LADDER_VIEW)
        fl, keep = to_dg_lists(dg, scene, rec, lists)
        fl2, keep2 = to_dg_lists(dg, scene, rec2, ladder)
        frames = (dg.DgFrameLists * 3)(fl, fl2, fl)
        owners = [hand_owners(dg, l, n_segs, scene.mobj_count()) for l in (lists, ladder, lists)]
        ctx = dg.Context(W, H, max_batch=3, slots=1)
        ctx.upload_scene(scene)
        if variant in sk.SMALL:                                      # refused by the binner like the reference's index panic; the slot stays usable
            for call in (lambda: ctx.draw_lists(0, frames), lambda: ctx.depth_lists(0, frames), lambda: ctx.label_lists(0, frames, owners)):
                with pytest.raises(dg.DoomGpuError, match="sky texture smaller than 256x128") as e:
                    call()
                assert e.value.code == dg.DG_ERR_RENDER
            other, other_owners, keep3 = other_batch_hand(dg, campath_mod, scene, W, H)
            want = dg.depth_lists_host(scene, W, H, other)
            for g, w in zip(ctx.depth_lists(0, other), want):
                _diff(g, w, f"{variant} {W}x{H}: a batch without sky after the refusal")
            ctx.close()
            continue
        names, np_wad = np_depth.SceneNames(dg, scene, wad, nf), nm.Wad(wad)
        colour = [nm.draw_lists(np_wad, "SKY1", W, H, v, l) for (v, l) in ((vd, lists), (vd2, ladder))]
        got = ctx.draw_lists(0, frames)
        for i, want in enumerate((colour[0], colour[1], colour[0])):
            bad = np.argwhere(np.any(got[i] != want, axis=2))
            assert len(bad) == 0, f"{variant} {W}x{H} frame {i} colour: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): gpu {got[i][bad[0][0], bad[0][1]]} numpy {want[bad[0][0], bad[0][1]]}"
        model = [models(names, W, H, frames[i], owners[i], scene.mobj_count()) for i in range(2)]
        model = [np.stack([model[i][j] for i in (0, 1, 0)]) for j in range(5)]
        for j, (g, plane) in enumerate(zip(ctx.depth_lists(0, frames) + ctx.label_lists(0, frames, owners), ("distance", "kind", "id", "cls", "boxes"))):
            _diff(g, model[j], f"{variant} {W}x{H} {plane} against the model")
        assert (model[1] == 3).any() and (model[1] == 0).any()
        assert ctx.fallbacks() == ZERO
        ctx.close()
        del keep, keep2
    scene.close()


def other_batch_hand(dg, campath_mod, scene, W, H):
    columns = []
    lists = {"renders": [wall("WALLA", 144, (33.0, -70.0, 47.0, 66.0), 0, W - 1, -41.0, 87.0, [(x, 0, H - 1, H, -1) for x in range(W)], columns)],
             "columns": columns, "visplanes": [], "order": [(0, 0)]}
    rec, _vd = view_dict(campath_mod, 7.0, -3.0, 0.3, 0.0)
    fl, keep = to_dg_lists(dg, scene, rec, lists)
    return (dg.DgFrameLists * 1)(fl), [np.array([dg.owner_tag(nl.MOBJ, 0)], dtype=np.uint32)], keep


@pytest.fixture(scope="module")
def holey_views(dg, oracle, wad1993, path1993):
    """(scene, [(W, H, views, oracle frames, host depth planes, host label outputs)]) of the synthetic map with holey SKY1 patches — computed
    once for the three front ends."""
    wad = sk.synth_holey_wad(wad1993)
    osc = oracle.Scene(wad, "e1m1")
    scene = dg.Scene(wad, "e1m1")
    out = []
    for (W, H, recs) in ((320, 200, path1993[0:960:60]), (1283, 97, path1993[[297, 728]])):
        views = dg.make_views(recs)
        n = len(views)
        frames = np.stack([np.frombuffer(osc.render(W, H, r), dtype=np.uint8).reshape(H, W, 3) for r in recs])
        depth = [np.empty((n, H, W), np.int16), np.empty((n, H, W), np.uint8)]
        labels = [np.empty((n, H, W), np.uint16), np.empty((n, H, W), np.uint8), np.empty((n, scene.mobj_count()), dtype=dg.LABEL_BOX_DTYPE)]
        for i in range(n):
            fl, owners = scene.build_lists_owners(W, H, views[i])
            one = (dg.DgFrameLists * 1)(fl)
            for dst, src in zip(depth + labels, list(dg.depth_lists_host(scene, W, H, one)) + list(dg.label_lists_host(scene, W, H, one, [owners]))):
                dst[i] = src[0]
        out.append((W, H, views, frames, depth, labels))
    osc.close()
    assert [len(o[2]) for o in out] == [16, 2] and all((o[4][1] == 3).any() for o in out)      # sky pixels in both batches
    yield scene, out
    scene.close()


@pytest.mark.parametrize("front_end", [1, 2, 3], ids=["host-lists", "device-column-walk", "device-seg-walk"])
def test_views_of_the_synthetic_map_with_a_holey_sky(dg, holey_views, front_end):
    scene, batches = holey_views
    for (W, H, views, frames, depth, labels) in batches:
        ctx = dg.Context(W, H, max_batch=len(views), slots=1, front_end=front_end)
        ctx.upload_scene(scene)
        got = ctx.render(views)
        assert ctx.timing(0)["front_end"] == front_end
        for i in range(len(views)):
            bad = np.argwhere(np.any(got[i] != frames[i], axis=2))
            assert len(bad) == 0, f"{W}x{H} view {i} front end {front_end}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"
        for g, w, plane in zip(ctx.render_depth(views), depth, ("distance", "kind")):
            _diff(g, w, f"{W}x{H} front end {front_end} {plane} against the host entry")
        for g, w, plane in zip(ctx.render_labels(views), labels, ("id", "cls", "boxes")):
            _diff(g, w, f"{W}x{H} front end {front_end} {plane} against the host entry")
        assert ctx.fallbacks() == ZERO
        ctx.close()
