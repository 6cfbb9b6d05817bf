"""CPU tier of tests/staging_cases.py: dg_depth_lists_host and dg_label_lists_host == the numpy models (np_depth, np_labels) on `ladder`
and `box_edges` at 64x40, 65x129 (a last band of one row) and 130x33 (three strips, one row past a box piece), byte for byte — and, from the
model alone, that the cases put what they claim where they claim it, so that no comparison passes vacuously:

  ladder      the span counts per column; each of flat, opaque wall, sky and holey wall is the visible owner of a pixel from a span index
              <= 15 and of one from an index >= 16; a pixel falls through a transparent texel of a span at index >= 16 onto a span at
              index <= 15, and one falls through a span at index <= 15 onto nothing.  On the hand WAD with the holey sky (sky_cases) the
              sky does both as well.
  box_edges   the whole-frame box out of four one-pixel runs, the single pixel, runs ending on row 31 / 127 and starting on 32 / 128, two
              runs in one column, an object in every strip, objects 0 and mobj_count - 1, a drawn object whose box is -1; the boxes'
              pixel counts add up to the map-object pixels of the frame.
"""
import numpy as np
import pytest

import np_depth
import np_labels as nl
import sky_cases
import staging_cases as sc
from test_edge_kats import to_dg_lists, view_dict
from test_labels_host import hand_owners

SIZES = [(64, 40), (65, 129), (130, 33)]


def _planes_equal(got, want, what):
    for name, g, w in zip(("distance", "kind", "id", "cls"), got, want):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): host {g[tuple(bad[0])]} model {w[tuple(bad[0])]}"


def run_case(dg, scene, names, campath_mod, W, H, view, lists, owners):
    """-> host (distance, kind, id, cls, boxes), model (the same five), tracker."""
    rec, _vd = view_dict(campath_mod, *view)
    fl, keep = to_dg_lists(dg, scene, rec, lists)
    frames = (dg.DgFrameLists * 1)(fl)
    d, k = [a[0] for a in dg.depth_lists_host(scene, W, H, frames)]
    i, c, b = [a[0] for a in dg.label_lists_host(scene, W, H, frames, [owners])]
    dist, kind, _tr = np_depth.depth_of_frame_lists(names, "SKY1", W, H, fl)
    ids, cls, boxes, tr, kind2 = nl.labels_of_frame_lists(names, "SKY1", W, H, fl, owners, scene.mobj_count())
    assert np.array_equal(kind, kind2)
    del keep
    return (d, k, i, c, b), (dist, kind, ids, cls, boxes), tr


@pytest.fixture(scope="module")
def worlds(dg, wad1993):
    """{which: (scene, model names, ladder texture names, segs)}: the light synthetic map, and the hand WAD with the holey sky."""
    import np_front_end as nf
    out = {}
    for which, wad, names in (("synth", wad1993, sc.SYNTH), ("holey", sky_cases.variant_wad("holey"), sc.HAND)):
        scene = dg.Scene(wad, "e1m1")
        out[which] = (scene, np_depth.SceneNames(dg, scene, wad, nf), names, len(nf.Map(wad, "e1m1").segs))
    yield out
    for (scene, *_r) in out.values():
        scene.close()


@pytest.fixture(scope="module")
def ladders(dg, campath_mod, worlds):
    out = {}
    for which, (scene, names, tex, n_segs) in worlds.items():
        for (W, H) in SIZES:
            lists = sc.ladder(W, H, tex)
            owners = hand_owners(dg, lists, n_segs, scene.mobj_count())
            out[(which, W, H)] = (lists,) + run_case(dg, scene, names, campath_mod, W, H, sc.LADDER_VIEW, lists, owners)
    return out


def test_ladder_host_entries_equal_the_models(ladders):
    assert len(ladders) == 6
    for (which, W, H), (_l, got, want, _tr) in ladders.items():
        _planes_equal(got[:4], want[:4], f"ladder {which} {W}x{H}")
        assert np.array_equal(got[4], want[4]), f"ladder {which} {W}x{H}: boxes"


def test_ladder_is_what_it_claims(ladders):
    for (which, W, H), (lists, _g, want, tr) in ladders.items():
        per_col = np.zeros(W, dtype=int)
        for c in lists["columns"]:
            per_col[c[0]] += 1
        for p in lists["visplanes"]:
            per_col[p["left"]:p["right"] + 1] += 1
        assert per_col.tolist() == [sc.ladder_count(x) for x in range(W)]
        assert {0, 1, 7, 8, 9, 15, 16, 17, 24, 33} == set(per_col.tolist())
        assert [int(per_col[x]) for x in (62, 63)] == [15, 16] and (W < 65 or per_col[64] == 17)
        slots = np.array(lists["slots"])
        kinds = slots % 4
        writer = tr.writer
        owner_slot = np.where(writer >= 0, slots[np.maximum(writer, 0)], -1)
        owner_kind = np.where(writer >= 0, kinds[np.maximum(writer, 0)], -1)
        cover = sc.ladder_cover(W, H, lists)
        # the binner drops none of the spans, so a span's index in its column is its slot: it skips a flat column whose clamped rows have
        # bottom - top <= 1 and a wall or sky column whose clamped top lies below its bottom (binner.cpp, visplanes.rs:99-101)
        for p in lists["visplanes"]:
            need = 0 if "SKY" in p["flat"] else 2
            assert all(min(b, H - 1) - max(t, 0) >= need for (t, b) in p["tb"]), f"{which} {W}x{H}: the binner skips a column of plane {p['flat']}"
        assert all(0 <= x < W and max(ct, 0) <= min(cb, H - 1) for (x, ct, cb, _b, _t) in lists["columns"]), f"{which} {W}x{H}: the binner skips a wall column"
        for k, name in ((sc.FLAT, "flat"), (sc.OPAQUE, "opaque wall"), (sc.SKY, "sky"), (sc.HOLEY, "holey wall")):
            assert ((owner_kind == k) & (owner_slot <= 15)).any(), f"{which} {W}x{H}: no {name} pixel from a staged span"
            assert ((owner_kind == k) & (owner_slot >= 16)).any(), f"{which} {W}x{H}: no {name} pixel from a span past the staging"
        assert (want[1][(owner_kind == sc.SKY)] == 3).all() and (want[1][owner_kind == sc.FLAT] == 2).all()
        high = cover[slots >= 16].any(axis=0)                       # some span at index >= 16 covers the pixel ...
        assert (high & (owner_slot >= 0) & (owner_slot <= 15)).any(), f"{which} {W}x{H}: nothing falls from index >= 16 onto index <= 15"
        assert (cover.any(axis=0) & ~high & (writer < 0)).any(), f"{which} {W}x{H}: nothing falls from index <= 15 onto nothing"
        if which == "holey":                                         # ... and with the holey sky, a SKY span lets a pixel through both ways
            sky_high = cover[(slots >= 16) & (kinds == sc.SKY)].any(axis=0)
            sky_low = cover[(slots <= 15) & (kinds == sc.SKY)].any(axis=0)
            assert (sky_high & (owner_slot >= 0) & (owner_slot <= 15) & ~cover[(slots >= 16) & (kinds != sc.SKY)].any(axis=0)).any()
            assert (sky_low & (writer < 0) & ~cover[kinds != sc.SKY].any(axis=0)).any()


@pytest.fixture(scope="module")
def boxes(dg, campath_mod, worlds):
    scene, names, _tex, n_segs = worlds["synth"]
    out = {}
    for (W, H) in SIZES:
        lists, owners, role = sc.box_edges(W, H, scene.mobj_count(), n_segs)
        out[(W, H)] = (lists, owners, role) + run_case(dg, scene, names, campath_mod, W, H, sc.BOX_VIEW, lists, owners)
    return out


def test_box_edges_host_entries_equal_the_models(boxes):
    for (W, H), (_l, _o, _r, got, want, _tr) in boxes.items():
        _planes_equal(got[:4], want[:4], f"box_edges {W}x{H}")
        bad = np.nonzero(got[4] != want[4])[0]
        assert len(bad) == 0, f"box_edges {W}x{H}: boxes differ, first for map object {bad[0]}: host {got[4][bad[0]]} model {want[4][bad[0]]}"


def test_box_edges_is_what_it_claims(boxes):
    for (W, H), (_l, owners, role, _g, (_d, _k, ids, cls, bx), _tr) in boxes.items():
        mobj = cls == nl.MOBJ
        own = lambda who: mobj & (ids == role[who])
        box = lambda who: tuple(int(bx[role[who]][f]) for f in ("pixels", "x0", "y0", "x1", "y1"))
        assert bx["pixels"].sum() == mobj.sum()
        assert box("corners") == (4, 0, 0, W - 1, H - 1) and role["corners"] == 0
        assert box("single")[0] == 1 and role["single"] == len(bx) - 1
        x1 = (5 * W) // 8
        assert own("upto31")[31, x1] and not own("upto31")[32, x1] and box("upto31")[4] == 31
        assert own("from32")[32, x1] and not own("from32")[31, x1] and box("from32")[2] == 32
        if H > 128:
            assert own("upto127")[127, x1 + 2] and box("upto127")[4] == 127 and own("from128")[128, x1 + 2] and box("from128")[2] == 128
        col = own("split")[:, W // 4]
        runs = np.flatnonzero(np.diff(np.concatenate([[0], col.astype(int), [0]])) == 1)
        assert len(runs) == 2 and own("between")[:, W // 4].sum() == 3
        assert all(own("everywhere")[:, s:s + 64].any() for s in range(0, W, 64))
        assert box("hidden") == (0, -1, -1, -1, -1) and (2 << 16 | role["hidden"]) in owners.tolist()
