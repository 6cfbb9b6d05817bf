"""CPU tier of the depth / surface-kind frame: dg_depth_lists_host (the binner + csrc/plane_core.h on the CPU, what the GPU path is
tested against in test_depth_gpu.py) must equal tests/np_depth.py byte for byte — the model that drives np_mappers.py with a patched
diminish_color and shares nothing with plane_core.h.

  whole frames    dg_build_lists output of the light map (seed 1993), the vanilla-shaped map (1995) and the hand-packed IWAD of
                  test_hand_wad.py: five views each at 160x100, one at 131x67 and one at 5x9 — masked walls, sprites, sky, and a sprite
                  whose transparent texels expose the wall behind it
  hand-built      tests/depth_cases.py: the vy == 0 row, bottom_y == top_y, uz0 == 0, x >= W, the 1-row skip, sky over a wall, an
                  all-transparent masked column, a 70-span column, 24 records per column
  errors          every error return of the host entry
  consistency     kind == 0 exactly where np_mappers' colour path wrote no pixel
"""
import ctypes

import numpy as np
import pytest

import depth_cases
import np_depth
from test_edge_kats import to_dg_lists, view_dict
from test_hand_wad import _views as hand_views, build_hand_iwad

SIZES = [(160, 100, 5), (131, 67, 1), (5, 9, 1)]         # (W, H, views)


def _assert_planes(got, want, what):
    for name, g, w in (("distance", got[0], want[0]), ("kind", got[1], want[1])):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): host {g[bad[0][0], bad[0][1]]} model {w[bad[0][0], bad[0][1]]}"


def _map_views(dg, campath_mod, which, wad1993, wad1995, path1993, path1995):
    """-> (wad, [dg_view ...]) of one of the three maps: path frames of the synthetic maps, the hand-packed IWAD's own views."""
    if which == "hand":
        wad = build_hand_iwad()
        sc = dg.Scene(wad, "e1m1")
        vs = hand_views(campath_mod, sc)
        arr = dg.make_views(np.stack([r[:8] for (r, _) in vs]))
        for k, (_, ts) in enumerate(vs):
            arr[k].timestamp = ts
        sc.close()
        return wad, [arr[k] for k in (2, 0, 3, 5, 6)]
    wad, path = (wad1993, path1993) if which == "light" else (wad1995, path1995)
    arr = dg.make_views(path[[0, 297, 500, 728, 900]])
    return wad, list(arr)


@pytest.fixture(scope="module")
def whole_frames(dg, campath_mod, wad1993, wad1995, path1993, path1995):
    """Per map: [(W, H, host planes, model planes, lists facts)] — computed once, shared by the tests below."""
    import np_front_end as nf
    out = {}
    for which in ("light", "vanilla", "hand"):
        wad, views = _map_views(dg, campath_mod, which, wad1993, wad1995, path1993, path1995)
        scene = dg.Scene(wad, "e1m1")
        names = np_depth.SceneNames(dg, scene, wad, nf)
        rows = []
        for (W, H, n) in SIZES:
            for v in views[:n]:
                fl = scene.build_lists(W, H, v)
                frames = (dg.DgFrameLists * 1)(fl)
                got = dg.depth_lists_host(scene, W, H, frames)
                dist, kind, tr = np_depth.depth_of_frame_lists(names, "SKY1", W, H, fl)
                facts = {"sprite": [], "masked": 0}
                for t in range(fl.n_order):
                    cmd = fl.order[t]
                    if cmd.kind != 0:
                        continue
                    r = fl.renders[cmd.index]
                    w, h, px = names.bitmaps[r.bitmap]
                    holes = any(texel is None for row in px for texel in row)
                    if r.bitmap in names.sprite_ids:
                        cover = np.zeros((H, W), dtype=bool)
                        for i in range(r.first_column, r.first_column + r.n_columns):
                            c = fl.columns[i]
                            if 0 <= c.x < W and c.clipped_top_y <= c.clipped_bottom_y:
                                cover[max(0, c.clipped_top_y):min(H - 1, c.clipped_bottom_y) + 1, c.x] = True
                        facts["sprite"].append((t, cover))
                    elif holes:
                        facts["masked"] += int((tr.writer == t).sum())
                rows.append((W, H, (got[0][0], got[1][0]), (dist, kind), tr, facts))
        scene.close()
        out[which] = rows
    return out


@pytest.mark.parametrize("which", ["light", "vanilla", "hand"])
def test_whole_frames_equal_the_model(whole_frames, which):
    rows = whole_frames[which]
    assert [(W, H) for (W, H, *_r) in rows] == [(160, 100)] * 5 + [(131, 67), (5, 9)]
    kinds_seen, sprite_px, masked_px = set(), 0, 0
    for (W, H, got, want, tr, facts) in rows:
        _assert_planes(got, want, f"{which} {W}x{H}")
        kinds_seen |= set(np.unique(want[1]).tolist())
        sprite_px += sum(int((tr.writer == t).sum()) for (t, _c) in facts["sprite"])
        masked_px += facts["masked"]
        assert (want[0][(want[1] == 0) | (want[1] == 3)] == 32767).all()
    assert {1, 2, 3} <= kinds_seen, kinds_seen                    # columns, flats and sky all own pixels
    assert sprite_px > 0 and masked_px > 0, (sprite_px, masked_px)   # sprites and masked walls (textures with holes) own pixels


def test_a_sprites_holes_expose_the_wall_behind_it(whole_frames):
    """Inside a sprite's columns and rows, pixels the sprite did not write (transparent texels) that an EARLIER column draw call owns: a
    wall behind it.  The two owners sit at different distances, in the host planes as in the model."""
    found = 0
    for which in ("hand", "light", "vanilla"):
        for (W, H, got, want, tr, facts) in whole_frames[which]:
            for (t, cover) in facts["sprite"]:
                own = cover & (tr.writer == t)
                behind = cover & (tr.writer >= 0) & (tr.writer < t) & (want[1] == 1)
                for x in np.nonzero(own.any(axis=0) & behind.any(axis=0))[0]:
                    d_sprite = set(got[0][own[:, x], x].tolist())
                    d_wall = set(got[0][behind[:, x], x].tolist())
                    assert len(d_sprite) == 1                     # z is a column constant
                    assert d_sprite.isdisjoint(d_wall), (which, W, H, t, x, d_sprite, d_wall)
                    found += 1
    assert found > 0, "no frame shows a wall through a sprite's transparent texels"


# ---- hand-built lists --------------------------------------------------------------------------------------------------------------

HAND_SIZES = {(64, 40): None, (5, 9): None, (131, 67): ("horizon", "masked_over_floor")}      # None: every case


@pytest.fixture(scope="module")
def hand_built(dg, campath_mod, wad1993):
    """{(W, H, name): (lists, view dict, host planes, model planes)}"""
    scene = dg.Scene(wad1993, "e1m1")
    out = {}
    for (W, H), only in HAND_SIZES.items():
        for name, v, lists in depth_cases.cases(W, H):
            if only and name not in only:
                continue
            rec, vd = view_dict(campath_mod, *v)
            fl, keep = to_dg_lists(dg, scene, rec, lists)
            frames = (dg.DgFrameLists * 1)(fl)
            got = dg.depth_lists_host(scene, W, H, frames)
            out[(W, H, name)] = (lists, vd, (got[0][0], got[1][0]), np_depth.depth_of_lists(wad1993, "SKY1", W, H, vd, lists))
    scene.close()
    return out


def test_hand_built_lists_equal_the_model(hand_built):
    assert len(hand_built) == 5 + 4 + 2
    for (W, H, name), (_l, _v, got, want) in hand_built.items():
        _assert_planes(got, want, f"{name} {W}x{H}")
        assert (want[1] != 0).any(), f"{name} {W}x{H} draws nothing"


def test_the_hand_built_lists_hit_their_corners(hand_built, wad1993):
    W, H = 64, 40
    dist, kind = hand_built[(W, H, "horizon")][2]
    w3 = W // 3
    # the vy == 0 row: -inf, +inf, NaN `as i16`
    assert kind[20, 0] == 2 and dist[20, 0] == -32768                      # wz = -41
    assert kind[20, w3 + 1] == 2 and dist[20, w3 + 1] == 32767              # wz = 87 (odd column: the plane reaches row 21)
    assert kind[20, 2 * w3 + 1] == 2 and dist[20, 2 * w3 + 1] == 0          # wz = 0: 0 / 0
    assert (np.unique(dist[kind == 2]) < 0).any()                           # negative distances are stored as they are
    # bottom - top == 0 and 1 are skipped, 2 and 3 are drawn: columns 0 .. 3 of the NUKAGE1 plane on its own
    lists = hand_built[(W, H, "horizon")][0]
    only_nukage = dict(lists, order=[(1, 3)])
    d1, k1 = np_depth.depth_of_lists(wad1993, "SKY1", W, H, hand_built[(W, H, "horizon")][1], only_nukage)
    assert (k1[:, 0] == 0).all() and (k1[:, 1] == 0).all() and (k1[:, 2] == 2).sum() == 3 and (k1[:, 3] == 2).sum() == 4
    # the sky plane over the wall: rows 0 .. x % 4 are sky, the wall shows below
    assert kind[0, 5] == 3 and dist[0, 5] == 32767 and kind[1, 5] == 3 and kind[2, 5] == 1 and dist[2, 5] != 32767
    # wall corners: a column at x >= W wrote nothing anywhere; the NaN row's owner differs between columns (HOLEY1 has holes)
    dist, kind = hand_built[(W, H, "wall_corners")][2]
    assert dist.shape == (H, W)
    lists = hand_built[(W, H, "wall_corners")][0]
    d2, k2 = np_depth.depth_of_lists(wad1993, "SKY1", W, H, hand_built[(W, H, "wall_corners")][1], dict(lists, order=[(0, 4)]))
    assert sorted(np.nonzero(k2.any(axis=0))[0].tolist()) == [W - 4, W - 1]  # of the seven columns only the two inside the frame
    # the masked column whose every texel is transparent keeps the floor's kind and distance
    lists, vd, (dist, kind), _ = hand_built[(W, H, "masked_over_floor")]
    floor_only = np_depth.depth_of_lists(wad1993, "SKY1", W, H, vd, dict(lists, order=[(1, 0)]))
    grate_only = np_depth.depth_of_lists(wad1993, "SKY1", W, H, vd, dict(lists, order=[(0, 0)]))
    empty_cols = [x for x in range(W) if not grate_only[1][:, x].any() and x not in range(W // 2, W // 2 + 5)]
    drawn_cols = [x for x in range(W) if grate_only[1][:, x].any()]
    assert empty_cols and drawn_cols
    for x in empty_cols:
        assert kind[20, x] == 2 and dist[20, x] == floor_only[0][20, x]
    # the 70-span column
    per_col = np.zeros(W, dtype=int)
    for c in hand_built[(W, H, "seventy")][0]["columns"]:
        per_col[c[0]] += 1
    assert per_col[21] == 70
    per_col = np.zeros(W, dtype=int)
    for c in hand_built[(W, H, "dense_strip")][0]["columns"]:
        per_col[c[0]] += 1
    assert per_col.min() > 16


def test_kind_zero_exactly_where_the_colour_path_wrote_nothing(hand_built, wad1993):
    for (W, H, name), (lists, vd, got, _w) in hand_built.items():
        if (W, H) != (64, 40):
            continue
        written = np_depth.written_mask(wad1993, "SKY1", W, H, vd, lists)
        assert np.array_equal(got[1] == 0, ~written), name
        assert (~written).any() or name in ("masked_over_floor", "seventy"), name


def test_either_output_may_be_left_out(dg, hand_built, campath_mod, wad1993):
    scene = dg.Scene(wad1993, "e1m1")
    name, v, lists = depth_cases.cases(64, 40)[0]
    rec, _vd = view_dict(campath_mod, *v)
    fl, keep = to_dg_lists(dg, scene, rec, lists)
    frames = (dg.DgFrameLists * 2)(fl, fl)
    d, k = dg.depth_lists_host(scene, 64, 40, frames, kind=False)
    assert k is None and np.array_equal(d[0], hand_built[(64, 40, name)][2][0]) and np.array_equal(d[1], d[0])
    d, k = dg.depth_lists_host(scene, 64, 40, frames, distance=False)
    assert d is None and np.array_equal(k[1], hand_built[(64, 40, name)][2][1])
    scene.close()


def test_every_error_return_of_the_host_entry(dg, campath_mod, wad1993):
    L = dg.lib()
    scene = dg.Scene(wad1993, "e1m1")
    name, v, lists = depth_cases.cases(64, 40)[0]
    rec, _vd = view_dict(campath_mod, *v)
    fl, keep = to_dg_lists(dg, scene, rec, lists)
    frames = (dg.DgFrameLists * 1)(fl)
    d = np.full((1, 40, 64), 77, dtype=np.int16)
    k = np.full((1, 40, 64), 77, dtype=np.uint8)
    dp, kp = d.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p)
    assert L.dg_depth_lists_host(None, 64, 40, frames, 1, dp, kp) == dg.DG_ERR_INVALID
    assert L.dg_depth_lists_host(scene._h, 64, 40, None, 1, dp, kp) == dg.DG_ERR_INVALID
    for (W, H) in ((0, 40), (64, 0), (-1, 40), (64, -3), (16385, 40), (64, 16385)):
        assert L.dg_depth_lists_host(scene._h, W, H, frames, 1, dp, kp) == dg.DG_ERR_INVALID, (W, H)
    assert L.dg_depth_lists_host(scene._h, 64, 40, frames, -1, dp, kp) == dg.DG_ERR_INVALID
    assert L.dg_last_error()
    assert (d == 77).all() and (k == 77).all()                     # nothing was written by a refused call
    assert L.dg_depth_lists_host(scene._h, 64, 40, frames, 0, dp, kp) == dg.DG_OK and (d == 77).all()
    assert L.dg_depth_lists_host(scene._h, 64, 40, frames, 1, None, None) == dg.DG_OK
    # malformed lists are the binner's errors: a draw command that names a missing record, a bitmap id out of range
    bad = (dg.DgFrameLists * 1)(fl)
    bad[0].n_renders = 0
    assert L.dg_depth_lists_host(scene._h, 64, 40, bad, 1, dp, kp) == dg.DG_ERR_INVALID
    assert b"frame 0" in L.dg_last_error()
    rs = (dg.DgBitmapRender * fl.n_renders)(*[fl.renders[i] for i in range(fl.n_renders)])
    rs[0].bitmap = 1 << 20
    bad = (dg.DgFrameLists * 1)(fl)
    bad[0].renders = rs
    assert L.dg_depth_lists_host(scene._h, 64, 40, bad, 1, dp, kp) == dg.DG_ERR_INVALID
    assert L.dg_depth_lists_host(scene._h, 64, 40, frames, 1, dp, kp) == dg.DG_OK and (k != 77).all()
    scene.close()


def test_the_binding_and_the_header_carry_the_depth_entry_points(dg):
    declared = dg.declared_symbols()
    for n in ("dg_depth_lists_host", "dg_submit_depth_views", "dg_render_depth_views", "dg_depth_lists", "dg_readback_depth"):
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert (dg.DG_KIND_NONE, dg.DG_KIND_COLUMN, dg.DG_KIND_FLAT, dg.DG_KIND_SKY, dg.DG_FE_DEPTH) == (0, 1, 2, 3, 5)
