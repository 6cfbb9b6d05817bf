"""CPU tier of the skies of tests/sky_cases.py: a sky bitmap with transparent texels (draw_sky writes only where the texel is Some,
src/renderer/visplanes.rs:74) and a sky smaller than 256x128.

  the WADs        the four variants decode as intended (numpy decoder) and the product's loader takes them
  colour          hand-built lists (sky_cases.sky_lists, and staging_cases.ladder on the hand WAD's textures) at 64x40 and 131x67 for
                  `holey` and `holey-gap`: oracle == numpy == tests/emul (emul_draw_lists: the binner and the kernel bodies on the CPU)
  depth, labels   dg_depth_lists_host and dg_label_lists_host == np_depth / np_labels on the same lists, three sizes
  small skies     `small` and `small-holey` are rendered by nothing: the reference indexes outside its bitmap there (no oracle, no model),
                  and the product's binner returns DG_ERR_RENDER ("sky texture smaller than 256x128") for a sky plane of such a bitmap.
                  That refusal is what is pinned, for the host entries and for tests/emul on lists and on views: the product never reaches
                  the outside-the-bitmap arms of raster_core.h through an entry point
  views           tests/emul on views of the hand WAD variants == the numpy renderer (np_front_end + np_mappers)
  whole views     the synthetic light map with holey SKY1 patches, 8 path views at 160x100: the numpy front end's lists == the product's
                  list builder; oracle == tests/emul (host lists, device column walk, device seg walk); oracle == numpy renderer on three of
                  them; depth and label host entries == the models on dg_build_lists output
  conditions      from the model alone, per hand-built frame: (a) a wall, (b) a flat, (c) nothing shows through a sky span, (d) an opaque sky
                  texel owns a pixel
"""
import numpy as np
import pytest

import emul_bind
import np_depth
import np_front_end as nf
import np_labels as nl
import np_mappers as nm
import sky_cases as sk
import staging_cases
from test_edge_kats import to_dg_lists, view_dict
from test_hand_wad import _views as hand_views, build_hand_iwad
from test_labels_host import hand_owners
from test_np_front_end import frame_lists

SIZES = [(64, 40), (131, 67), (65, 129)]
DRAWN = [v for v in sk.VARIANTS if v not in sk.SMALL]
PATH_VIEWS = [0, 100, 297, 323, 500, 623, 728, 900]


def _first_bad(got, want):
    bad = np.argwhere(got != want if got.ndim == 2 else np.any(got != want, axis=2))
    return "" if len(bad) == 0 else f"{len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): {got[bad[0][0], bad[0][1]]} against {want[bad[0][0], bad[0][1]]}"


def test_the_variants_are_what_they_claim(dg):
    for name in sk.VARIANTS:
        wad = sk.variant_wad(name)
        w, h, px = nm.Wad(wad).texture("SKY1")
        assert (w, h) == ((128, 64) if name in sk.SMALL else (256, 128))
        holes = np.array([[t is None for t in row] for row in px])
        if name in sk.HOLEY:
            assert holes[:, 100:104].all() and holes[60:62, :].all()                      # whole columns, whole rows
            assert holes[0:8, 0:8].all() and not holes[0:8, 8:16].any() and not holes[8:16, 0:8].any() and holes[8:16, 8:16].all()     # the checker
        else:
            assert not holes.any()
        if name == "holey-gap":
            assert holes[:, 128:192].all() and not holes[0:8, 200:208].any()           # tx 128..191: no patch covers them
        if name == "holey":
            assert not holes[:, 128:192].all()
        sc = dg.Scene(wad, "e1m1")                                                         # the product's loader takes it
        assert sc.mobj_count() == 4
        sc.close()


# ---- hand-built lists ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand_built(dg, campath_mod):
    """{(variant, W, H): dict(lists, rec, colour (numpy), emul colour, host depth + labels, model depth + labels, tracker)} for the two
    256x128 variants — computed once."""
    out = {}
    for name in DRAWN:
        wad = sk.variant_wad(name)
        scene = dg.Scene(wad, "e1m1")
        es = emul_bind.EmulScene(wad)
        names = np_depth.SceneNames(dg, scene, wad, nf)
        np_wad = nm.Wad(wad)
        n_segs = len(nf.Map(wad, "e1m1").segs)
        for (W, H) in SIZES:
            lists = sk.sky_lists(W, H)
            rec, vd = view_dict(campath_mod, *sk.SKY_VIEW)
            fl, keep = to_dg_lists(dg, scene, rec, lists)
            frames = (dg.DgFrameLists * 1)(fl)
            owners = hand_owners(dg, lists, n_segs, scene.mobj_count())
            host = [a[0] for a in dg.depth_lists_host(scene, W, H, frames)] + [a[0] for a in dg.label_lists_host(scene, W, H, frames, [owners])]
            ids, cls, boxes, tr, kind = nl.labels_of_frame_lists(names, "SKY1", W, H, fl, owners, scene.mobj_count())
            dist, kind2, _tr = np_depth.depth_of_frame_lists(names, "SKY1", W, H, fl)
            assert np.array_equal(kind, kind2)
            emul = np.frombuffer(es.draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)
            out[(name, W, H)] = {"lists": lists, "rec": rec, "vd": vd, "colour": nm.draw_lists(np_wad, "SKY1", W, H, vd, lists), "emul": emul, "host": host,
                                 "model": [dist, kind, ids, cls, boxes], "tr": tr}
            del keep
        scene.close()
    return out


@pytest.mark.parametrize("variant", DRAWN)
def test_colour_oracle_equals_numpy_on_the_hand_built_lists(oracle, hand_built, variant):
    """oracle == numpy == tests/emul (the binner and the kernel bodies on the given lists) at 64x40 and 131x67; emul == numpy at 65x129."""
    assert variant not in sk.SMALL                                   # the reference would index outside its bitmap: never the oracle
    osc = oracle.Scene(sk.variant_wad(variant), "e1m1")
    for (W, H) in SIZES[:2]:
        c = hand_built[(variant, W, H)]
        got = np.frombuffer(osc.draw_lists(W, H, c["rec"], c["lists"]), dtype=np.uint8).reshape(H, W, 3)
        assert not _first_bad(got, c["colour"]), f"{variant} {W}x{H} oracle against numpy: {_first_bad(got, c['colour'])}"
        assert not _first_bad(c["emul"], c["colour"]), f"{variant} {W}x{H} emul against numpy: {_first_bad(c['emul'], c['colour'])}"
    c = hand_built[(variant, *SIZES[2])]
    assert not _first_bad(c["emul"], c["colour"]), f"{variant} 65x129 emul against numpy: {_first_bad(c['emul'], c['colour'])}"
    osc.close()


@pytest.mark.parametrize("variant", DRAWN)
def test_colour_oracle_numpy_and_emul_agree_on_the_ladder(dg, oracle, campath_mod, variant):
    """staging_cases.ladder on the hand WAD's textures: up to 33 spans of all four kinds per column, sky spans with holes among them."""
    wad = sk.variant_wad(variant)
    scene, osc, es, np_wad = dg.Scene(wad, "e1m1"), oracle.Scene(wad, "e1m1"), emul_bind.EmulScene(wad), nm.Wad(wad)
    for (W, H) in SIZES[:2]:
        lists = staging_cases.ladder(W, H, staging_cases.HAND)
        rec, vd = view_dict(campath_mod, *staging_cases.LADDER_VIEW)
        fl, keep = to_dg_lists(dg, scene, rec, lists)
        want = nm.draw_lists(np_wad, "SKY1", W, H, vd, lists)
        got = np.frombuffer(osc.draw_lists(W, H, rec, lists), dtype=np.uint8).reshape(H, W, 3)
        assert not _first_bad(got, want), f"{variant} {W}x{H} oracle against numpy: {_first_bad(got, want)}"
        got = np.frombuffer(es.draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)
        assert not _first_bad(got, want), f"{variant} {W}x{H} emul against numpy: {_first_bad(got, want)}"
        assert want.any()
        del keep
    osc.close()
    scene.close()


@pytest.mark.parametrize("variant", sk.SMALL)
def test_a_small_sky_is_refused_on_the_hand_built_lists(dg, campath_mod, variant):
    """The binner refuses a sky plane of a bitmap smaller than 256x128 (binner.cpp), as the reference panics: the host
    entries return DG_ERR_RENDER and tests/emul, which bins with the same function, refuses the lists too."""
    wad = sk.variant_wad(variant)
    scene, es = dg.Scene(wad, "e1m1"), emul_bind.EmulScene(wad)
    n_segs = len(nf.Map(wad, "e1m1").segs)
    for (W, H) in SIZES:
        lists = sk.sky_lists(W, H)
        rec, _vd = view_dict(campath_mod, *sk.SKY_VIEW)
        fl, keep = to_dg_lists(dg, scene, rec, lists)
        frames = (dg.DgFrameLists * 1)(fl)
        owners = hand_owners(dg, lists, n_segs, scene.mobj_count())
        for call in (lambda: dg.depth_lists_host(scene, W, H, frames), lambda: dg.label_lists_host(scene, W, H, frames, [owners])):
            with pytest.raises(dg.DoomGpuError, match="sky texture smaller than 256x128") as e:
                call()
            assert e.value.code == dg.DG_ERR_RENDER
        with pytest.raises(RuntimeError, match="sky texture smaller than 256x128"):
            es.draw_lists(W, H, fl)
        del keep
    scene.close()


def test_depth_and_labels_host_entries_equal_the_models(hand_built):
    assert len(hand_built) == 6
    for (variant, W, H), c in hand_built.items():
        for what, g, w in zip(("distance", "kind", "id", "cls"), c["host"], c["model"]):
            assert not _first_bad(g, w), f"{variant} {W}x{H} {what}, host against model: {_first_bad(g, w)}"
        assert np.array_equal(c["host"][4], c["model"][4]), f"{variant} {W}x{H}: boxes"
        assert not c["colour"][c["model"][1] == 0].any()             # kind 0: the colour path wrote nothing there either


def test_every_hand_built_frame_meets_its_conditions(hand_built):
    for (variant, W, H), c in hand_built.items():
        lists, tr, (dist, kind, ids, cls, _b), colour = c["lists"], c["tr"], c["model"], c["colour"]
        writer = tr.writer
        sky1, sky2 = sk.sky_cover(W, H, lists, 1), sk.sky_cover(W, H, lists, 2)
        where = f"{variant} {W}x{H}"
        assert variant in sk.HOLEY
        assert (sky1 & (writer == sk.T_WALL)).any(), f"{where}: (a) no wall shows through the sky"
        assert (kind[sky1 & (writer == sk.T_WALL)] == 1).all()
        assert (sky1 & (writer == sk.T_FLAT)).any(), f"{where}: (b) no flat shows through the sky"
        assert (kind[sky1 & (writer == sk.T_FLAT)] == 2).all()
        nothing = (sky1 | sky2) & (writer < 0)
        assert nothing.any(), f"{where}: (c) no pixel under a sky span stays unwritten"
        assert (kind[nothing] == 0).all() and (cls[nothing] == 0).all() and (dist[nothing] == 32767).all() and not colour[nothing].any()
        assert (sky2 & (writer == sk.T_MASKED)).any(), f"{where}: the masked wall does not show through the second sky plane"
        owned = (writer == sk.T_SKY) | (writer == sk.T_SKY2)
        assert owned.any(), f"{where}: (d) no sky texel owns a pixel"
        assert (kind[owned] == 3).all() and (cls[owned] == nl.SKY).all() and (dist[owned] == 32767).all() and (ids[owned] == 0).all()
        # the masked wall drawn after the first sky plane: it owns pixels over the sky, and the sky shows through its holes
        masked = np.zeros((H, W), dtype=bool)
        r = lists["renders"][1]
        for (x, ct, cb, _by, _ty) in lists["columns"][r["first_column"]:r["first_column"] + r["n_columns"]]:
            masked[ct:cb + 1, x] = True
        assert (masked & sky1 & ~sky2 & (writer == sk.T_MASKED)).any() and (masked & ~sky2 & (writer == sk.T_SKY)).any(), where


# ---- views of the hand WAD variants through the product's bodies on the CPU -----------------------------------------------------------------

@pytest.mark.parametrize("variant", sk.VARIANTS)
def test_emul_equals_the_numpy_renderer_on_views_of_the_hand_wad(dg, campath_mod, variant):
    """tests/emul (host lists + kernel bodies, and the device column walk's bodies) against np_front_end + np_mappers:
    three views of the hand map that look at room B's sky ceiling, through the masked portal and from inside."""
    wad = sk.variant_wad(variant)
    sc = dg.Scene(wad, "e1m1")
    es = emul_bind.EmulScene(wad)
    if variant in sk.SMALL:                                          # refused like the reference's index panic, by every front end's bodies
        rec, ts = hand_views(campath_mod, sc)[2]
        for call in (es.render, es.render_fe):
            with pytest.raises(RuntimeError, match="sky texture smaller than 256x128"):
                call(160, 100, rec, ts)
        sc.close()
        return
    np_map, np_wad, things, sprites = nf.Map(wad, "e1m1"), nm.Wad(wad), nf.load_things(wad, "e1m1"), nf.SpriteTable(wad)
    W, H = 160, 100
    differs = 0
    for k in (0, 2, 3):
        rec, ts = hand_views(campath_mod, sc)[k]
        view = {"x": rec[0], "y": rec[1], "angle": rec[2], "cos": rec[3], "sin": rec[4], "cos_neg": rec[5], "sin_neg": rec[6], "floor_height": rec[7]}
        want = nf.render_frame(np_map, things, sprites, np_wad, nm, W, H, view, timestamp=ts)
        got = np.frombuffer(es.render(W, H, rec, ts)[0], dtype=np.uint8).reshape(H, W, 3)
        assert not _first_bad(got, want), f"{variant} view {k}, host lists: {_first_bad(got, want)}"
        got, st = es.render_fe(W, H, rec, ts)
        got = np.frombuffer(got, dtype=np.uint8).reshape(H, W, 3)
        assert not _first_bad(got, want) and st[3] == 0 and st[4] == 1, f"{variant} view {k}, device column walk: {_first_bad(got, want)} {st}"
        rc, st = es.fs_frame(W, H, rec, ts)
        assert rc == 0, (variant, k, rc, st)
        if k == 2:                                                   # the variant's sky is in the frame: the hand WAD's own sky gives another one
            differs += int(np.any(want != nf.render_frame(np_map, things, sprites, nm.Wad(build_hand_iwad()), nm, W, H, view, timestamp=ts), axis=2).sum())
    sc.close()
    assert differs > 200, differs


# ---- the synthetic map with a holey sky ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_holey(wad1993):
    return sk.synth_holey_wad(wad1993)


def test_synthetic_holey_views(dg, oracle, wad1993, oracle_scene1993, synth_holey, path1993):
    W, H = 160, 100
    w, h, px = nm.Wad(synth_holey).texture("SKY1")
    assert (w, h) == (256, 128) and px[60][5] is None and px[3][101] is None and px[0][0] is None and px[0][8] is not None
    osc = oracle.Scene(synth_holey, "e1m1")
    es = emul_bind.EmulScene(synth_holey)
    scene = dg.Scene(synth_holey, "e1m1")
    names = np_depth.SceneNames(dg, scene, synth_holey, nf)
    np_map, np_wad, things, sprites = nf.Map(synth_holey, "e1m1"), nm.Wad(synth_holey), nf.load_things(synth_holey, "e1m1"), nf.SpriteTable(synth_holey)
    views = dg.make_views(path1993[PATH_VIEWS])
    through = sky_px = 0
    for n, i in enumerate(PATH_VIEWS):
        r = path1993[i]
        # the numpy front end's lists against the product's list builder (as tests/test_np_front_end.py compares them)
        calls = nf.per_seg_calls(np_map, W, H, {"x": r[0], "y": r[1], "cos_neg": r[5], "sin_neg": r[6], "floor_height": r[7]})
        columns, visplanes = nf.column_loops(W, H, calls)
        renders, planes, order = frame_lists(es, W, H, r)
        first_plane = next((k for k, (kind, _) in enumerate(order) if kind == 1), len(order))
        want_inline = [cols for c, cols in zip(calls, columns) if (c["flags"] & nf.HAS_TEXTURE) and not (c["flags"] & (nf.IS_TWO_SIDED_MIDDLE_WALL | nf.ONLY_OCCLUSIONS)) and cols]
        assert [renders[idx] for kind, idx in order[:first_plane]] == want_inline, f"frame {i}: inline wall columns differ"
        assert [(l, rr, tb) for (_, _, l, rr, tb) in visplanes] == planes, f"frame {i}: visplanes differ"
        # whole frames: oracle == the product's bodies on the CPU, all three front ends
        ref = osc.render(W, H, r)
        assert es.render(W, H, r, 0.0)[0] == ref, f"frame {i}: host lists"
        got, st = es.render_fe(W, H, r, 0.0)
        assert got == ref and st[3] == 0 and st[4] == 1, f"frame {i}: device column walk {st}"
        rc, st = es.fs_frame(W, H, r, 0.0)
        assert rc == 0, (i, rc, st)
        want = np.frombuffer(ref, dtype=np.uint8).reshape(H, W, 3)
        if n % 3 == 0:                                               # oracle == the numpy renderer (pure-Python pixel loops: three views)
            view = {"x": r[0], "y": r[1], "angle": r[2], "cos": r[3], "sin": r[4], "cos_neg": r[5], "sin_neg": r[6], "floor_height": r[7]}
            got = nf.render_frame(np_map, things, sprites, np_wad, nm, W, H, view)
            assert not _first_bad(got, want), f"frame {i} numpy against oracle: {_first_bad(got, want)}"
        # depth and labels: host entries == the models on dg_build_lists output
        fl, owners = scene.build_lists_owners(W, H, views[n])
        frames = (dg.DgFrameLists * 1)(fl)
        host = [a[0] for a in dg.depth_lists_host(scene, W, H, frames)] + [a[0] for a in dg.label_lists_host(scene, W, H, frames, [owners])]
        ids, cls, boxes, tr, kind = nl.labels_of_frame_lists(names, "SKY1", W, H, fl, owners, scene.mobj_count())
        dist, _k, _t = np_depth.depth_of_frame_lists(names, "SKY1", W, H, fl)
        for what, g, wnt in zip(("distance", "kind", "id", "cls"), host, (dist, kind, ids, cls)):
            assert not _first_bad(g, wnt), f"frame {i} {what}, host against model: {_first_bad(g, wnt)}"
        assert np.array_equal(host[4], boxes)
        # what the holes show: against the same view of the map with its opaque sky
        opaque = np.frombuffer(oracle_scene1993.render(W, H, r), dtype=np.uint8).reshape(H, W, 3)
        through += int(np.any(want != opaque, axis=2).sum())
        sky_px += int((kind == 3).sum())
    assert through > 2000 and sky_px > 2000, (through, sky_px)
    scene.close()
    osc.close()
