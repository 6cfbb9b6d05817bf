"""CPU tier of the map-object markers on the map frames: dg_map_thing_lines, dg_ego_map_things_host and
dg_floor_map_things_host against the numpy restatement (np_map_things over np_ego / np_floor_map), byte for byte, on the cases of
map_thing_cases.py at 64x48, 333x77 and 16x16; and tests/map_things/map_things_host_main.cpp — the kernels' things phase as a host loop
for every band height against the literal rule — as a stand-alone program under AddressSanitizer + UBSan.

Every positive case is first held against itself: on the model's 64x48 frame each shown marker keeps a pixel no later line covers, so a
frame without markers cannot pass.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import floor_map_cases as fc
import map_thing_cases as mc
import mobj_fx as mf
import np_ego as ng
import np_map_things as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSITIVE = [c for c in mc.CASES if c["shown"]]


@pytest.fixture(scope="module")
def scenes(dg):
    out = {w: fc.open_scene(dg, w) for w in ("light", "hand")}
    yield out
    for sc in out.values():
        sc.close()


def _set(scenes, c):
    sc = scenes[c["world"]]
    sc.set_map_markers(mc.table(c["world"], c["marked"]))
    return sc


def _lines(dg, sc, c, W, H):
    return [tuple(r) for r in dg.map_thing_lines(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), mc.state_of(c), mc.poses_of(c)).tolist()]


def _ego(dg, sc, c, W, H):
    return dg.ego_map_things_host(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c), mc.state_of(c), mc.poses_of(c))


def _floor(dg, sc, c, W, H):
    return dg.floor_map_things_host(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c), mc.state_of(c), None, mc.poses_of(c))


@pytest.mark.parametrize("c", POSITIVE, ids=lambda c: c["name"])
def test_every_shown_marker_of_a_positive_case_keeps_a_pixel_on_the_model(c):
    W, H = mc.SIZES[0]
    view = fc.na.libm_view(*c["view"])
    things, table = mc.things_of(c["world"]), mc.table(c["world"], c["marked"])
    shown = nt.shown_objects(things, table, mc.hidden_of(c), c["poses"])
    assert {i for i, *_ in shown} == c["shown"]
    tl = mc.model_lines(c, W, H)
    lines = nt.all_lines(fc.model_of(c["world"]).ego, W, H, view, c["scale"], c["flags"], fc.mask_row(c), tl)
    first = len(lines) - len(tl) - (3 if c["flags"] & ng.ARROW else 0)
    own = nt.owners(lines, W, H)
    at = first
    for i, x, y, a in shown:                                                    # the object's lines are lines[at : at + n]
        n = len(nt.marker_segments(x, y, a, table[i][0], table[i][2]))
        assert n > 0 and ((own >= at) & (own < at + n)).any(), (c["name"], i)
        at += n
    assert at == first + len(tl)


@pytest.mark.parametrize("size", mc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lines_and_frames_equal_the_model(dg, scenes, size):
    W, H = size
    differ = 0
    for c in mc.CASES:
        sc = _set(scenes, c)
        assert _lines(dg, sc, c, W, H) == mc.model_lines(c, W, H), (c["name"], W, H)
        got, want = _ego(dg, sc, c, W, H), mc.model_ego(c, W, H)
        assert np.array_equal(got, want), (c["name"], W, H, int((got != want).any(axis=2).sum()))
        got, want = _floor(dg, sc, c, W, H), mc.model_floor(c, W, H)
        assert np.array_equal(got, want), (c["name"], W, H, int((got != want).any(axis=2).sum()))
        plain = dg.ego_map_host(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c))
        assert bool(c["shown"]) or np.array_equal(_ego(dg, sc, c, W, H), plain), c["name"]    # nothing shown: the plain frame
        plain_floor = dg.floor_map_host(sc, W, H, fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c))
        differ += int(not np.array_equal(_ego(dg, sc, c, W, H), plain) or not np.array_equal(_floor(dg, sc, c, W, H), plain_floor))   # (a black marker shows on the floor only)
    assert differ >= (len(POSITIVE) if size == mc.SIZES[0] else 4)


def test_the_default_table_on_the_light_world(dg, scenes):
    """Forty objects, most of them marked, the whole level in the frame and a close-up: more lines than one case's three objects give."""
    sc = scenes["light"]
    table = mc.default_table("light")
    sc.set_map_markers(table)
    things = mc.things_of("light")
    for (x, y, a), scale, flags in ((fc.P0, 0.05, fc.R | fc.A), (fc.P1, 0.25, 0), (fc.P2, 1.0, fc.R)):
        for W, H in ((333, 77), (64, 48)):
            c = fc.case("default", "light", x, y, a, 0.0, scale, flags)
            view = fc.na.libm_view(*c["view"])
            tl = nt.thing_lines(W, H, view, scale, flags, things, table)
            got = dg.map_thing_lines(sc, W, H, fc.view_of(dg, c), (scale, flags))
            assert [tuple(r) for r in got.tolist()] == tl and len(tl) > 60
            assert np.array_equal(dg.ego_map_things_host(sc, W, H, fc.view_of(dg, c), (scale, flags)), nt.ego_frame(fc.model_of("light").ego, W, H, view, scale, flags, None, tl))
            assert np.array_equal(dg.floor_map_things_host(sc, W, H, fc.view_of(dg, c), (scale, flags)),
                                  nt.floor_frame(fc.model_frame(c, W, H), fc.model_of("light").ego, W, H, view, scale, flags, None, tl))


def test_no_table_and_all_flags_0_equal_the_plain_host_functions(dg, scenes):
    W, H = 64, 48
    for c in (mc.BY_NAME["hand_whole_3"], mc.BY_NAME["light_near_7"]):
        sc = scenes[c["world"]]
        v, p, m = fc.view_of(dg, c), (c["scale"], c["flags"]), fc.mask_row(c)
        plain_ego, plain_floor = dg.ego_map_host(sc, W, H, v, p, m), dg.floor_map_host(sc, W, H, v, p, m)
        n = sc.mobj_count()
        for table in (None, [(16, mc.rgb_of(i), 0) for i in range(n)]):
            sc.set_map_markers(table)
            assert len(dg.map_thing_lines(sc, W, H, v, p)) == 0
            assert np.array_equal(dg.ego_map_things_host(sc, W, H, v, p, m), plain_ego) and np.array_equal(dg.floor_map_things_host(sc, W, H, v, p, m), plain_floor)
        _set(scenes, c)
        assert not np.array_equal(dg.ego_map_things_host(sc, W, H, v, p, m), plain_ego) and not np.array_equal(dg.floor_map_things_host(sc, W, H, v, p, m), plain_floor)


def test_later_pose_wins(dg, scenes):
    c = mc.BY_NAME["later_pose_wins"]
    sc = _set(scenes, c)
    W, H = 64, 48
    last = dict(c, poses=[c["poses"][-1]])
    first = dict(c, poses=[c["poses"][0]])
    assert _lines(dg, sc, c, W, H) == _lines(dg, sc, last, W, H) == mc.model_lines(last, W, H)
    assert _lines(dg, sc, c, W, H) != _lines(dg, sc, first, W, H)
    assert np.array_equal(_ego(dg, sc, c, W, H), _ego(dg, sc, last, W, H)) and not np.array_equal(_ego(dg, sc, c, W, H), _ego(dg, sc, first, W, H))


def test_a_state_entry_a_scene_state_and_a_thinkers_null_state_each_hide_the_object(dg):
    W, H = 64, 48
    # a state entry of -1, and the scene's state of -1 (the hand world; a later entry with a frame shows the object again)
    sc = fc.open_scene(dg, "hand")
    c = mc.BY_NAME["state_entry_hides"]
    sc.set_map_markers(mc.table("hand", c["marked"]))
    base = dict(c, mobjs=[])
    all_lines = _lines(dg, sc, base, W, H)
    hidden = _lines(dg, sc, c, W, H)
    assert hidden == mc.model_lines(c, W, H) and len(hidden) == len(all_lines) - 5 and hidden == all_lines[5:]
    sc.set_mobj_state(0, None)
    assert _lines(dg, sc, base, W, H) == hidden == mc.model_lines(base, W, H, scene_hidden={0})
    assert np.array_equal(_ego(dg, sc, base, W, H), mc.model_ego(base, W, H, scene_hidden={0}))
    assert np.array_equal(_floor(dg, sc, base, W, H), mc.model_floor(base, W, H, scene_hidden={0}))
    again = mc.BY_NAME["later_state_entry_shows"]
    assert _lines(dg, sc, again, W, H) == all_lines == mc.model_lines(again, W, H, scene_hidden={0})
    sc.close()
    # a thinker's S_NULL: a barrel's death chain ends in state 0 (mobj_fx.STATES 3, 4, 5, then 0)
    wad = mf.fx_wad()
    sc = dg.Scene(wad, "e1m1")
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    sc.mobj_event(mf.KILL, mf.ts(10))
    sim = mf.Sim(wad, events=[(mf.KILL, 10)])
    things = nt.read_things(wad)
    table = [(12, mc.rgb_of(i), nt.BOX | nt.HEADING) for i in range(len(things))]
    sc.set_map_markers(table)
    model = ng.EgoModel(wad)
    for T in (5, 40):
        null = {i for i, s in enumerate(sim.shown(T)) if s == "null"}
        assert bool(null) == (T == 40)
        x, y, a = fc.P0
        v = dg.DgView(x, y, a, 0, 0, 0, 0, 0, mf.ts(T), 0)
        view = fc.na.libm_view(x, y, a)
        tl = nt.thing_lines(W, H, view, 0.05, fc.R, things, table, null)
        got = dg.map_thing_lines(sc, W, H, v, (0.05, fc.R))
        assert [tuple(r) for r in got.tolist()] == tl and len(tl) == 5 * (len(things) - len(null))
        assert np.array_equal(dg.ego_map_things_host(sc, W, H, v, (0.05, fc.R)), nt.ego_frame(model, W, H, view, 0.05, fc.R, None, tl))
    # ... and a view's entry wins over the thinker
    first_null = min(null)
    got = dg.map_thing_lines(sc, W, H, v, (0.05, fc.R), ([], [(first_null, 0, 0)]))
    assert [tuple(r) for r in got.tolist()] == nt.thing_lines(W, H, view, 0.05, fc.R, things, table, null - {first_null})
    sc.close()


def test_positions_at_the_edge_of_the_rule(dg, scenes):
    W, H = 64, 48
    c = mc.BY_NAME["pose_at_32768"]
    sc = _set(scenes, c)
    got = _lines(dg, sc, c, W, H)
    assert len(got) == 5 and {l[4] for l in got} == {mc.rgb_of(0)} and got == mc.model_lines(c, W, H)      # 32768.0 draws; 32768.5 and NaN hide
    assert _ego(dg, sc, c, W, H).any()
    c = mc.BY_NAME["pose_beyond"]
    sc = _set(scenes, c)
    assert _lines(dg, sc, c, W, H) == [] and not _ego(dg, sc, c, W, H).any()
    c = mc.BY_NAME["heading_not_finite"]
    sc = _set(scenes, c)
    assert len(_lines(dg, sc, c, W, H)) == 4 + 4 + 4                                                        # three boxes, no heading line


def test_radius_0_is_one_point(dg, scenes):
    c = mc.BY_NAME["radius_0"]
    sc = _set(scenes, c)
    W, H = 64, 48
    got = _lines(dg, sc, c, W, H)
    assert len(got) == 5 and len({l[:2] for l in got} | {l[2:4] for l in got}) == 1
    frame = _ego(dg, sc, c, W, H)
    rgb = mc.rgb_of(0)
    assert int((frame == [rgb & 255, (rgb >> 8) & 255, rgb >> 16]).all(axis=2).sum()) == 1


def test_a_marker_over_a_line_and_under_the_arrow(dg, scenes):
    c = mc.BY_NAME["over_a_line_under_the_arrow"]
    sc = _set(scenes, c)
    W, H = 64, 48
    view = fc.na.libm_view(*c["view"])
    ego = fc.model_of("hand").ego
    walls = ego.lines_for(W, H, view, c["scale"], 0)
    tl = mc.model_lines(c, W, H)
    arrow = ng.arrow(W, H, view, c["scale"], False)
    on_walls, on_things, on_arrow = nt.owners(walls, W, H) >= 0, nt.owners(tl, W, H) >= 0, nt.owners(arrow, W, H) >= 0
    assert (on_walls & on_things & ~on_arrow).any() and (on_things & on_arrow).any()                         # the case is what its name says
    frame = _ego(dg, sc, c, W, H)
    assert np.array_equal(frame, mc.model_ego(c, W, H))
    rgb = mc.rgb_of(2)
    marker = (frame == [rgb & 255, (rgb >> 8) & 255, rgb >> 16]).all(axis=2)
    yellow = (frame == [255, 255, 0]).all(axis=2)
    assert marker[on_walls & on_things & ~on_arrow].all() and yellow[on_things & on_arrow].all()


def test_an_object_exactly_at_the_player(dg, scenes):
    c = mc.BY_NAME["at_the_player"]
    sc = _set(scenes, c)
    W, H = 64, 48
    got = _lines(dg, sc, c, W, H)
    assert got[4][:2] == (W // 2, H // 2)                                                                    # the heading starts at the player's pixel
    assert np.array_equal(_ego(dg, sc, c, W, H), mc.model_ego(c, W, H))


def test_every_error_return(dg, scenes, wad1993):
    L = dg.lib()
    sc = scenes["hand"]
    n = sc.mobj_count()
    M = dg.DgMapMarker
    good = (M * n)(*[M(16, 0x123456, 3)] * n)
    assert L.dg_scene_set_map_markers(sc._h, good, n) == dg.DG_OK
    v, p = dg.DgView(352.5, 250.0, 0.1, 0, 0, 0, 0, 0, 0, 0), dg.DgEgoMap(0.05, 3)
    bv, bp = ctypes.byref(v), ctypes.byref(p)
    P = lambda a: a.ctypes.data_as(dg._P)
    img = np.zeros((48, 64, 3), np.uint8)
    count = L.dg_map_thing_lines(sc._h, 64, 48, bv, bp, None, None, None, 0)
    assert count == 5 * n

    def table_refused(arr, k):
        assert L.dg_scene_set_map_markers(sc._h, arr, k) == dg.DG_ERR_INVALID
        assert L.dg_map_thing_lines(sc._h, 64, 48, bv, bp, None, None, None, 0) == count               # the table set before stands

    for bad in (M(-1, 0, 1), M(1025, 0, 1), M(16, 0x1000000, 1), M(16, 0, 4), M(16, 0, 0x80000001)):
        table_refused((M * n)(*([M(16, 0, 1)] * (n - 1) + [bad])), n)
    table_refused(good, n - 1)
    table_refused(good, n + 1)
    table_refused(good, 0)
    table_refused(None, n)
    assert L.dg_scene_set_map_markers(None, good, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_set_map_markers(sc._h, (M * n)(*[M(1024, 0xffffff, 3), M(0, 0, 0)] * (n // 2)), n) == dg.DG_OK
    assert L.dg_scene_set_map_markers(sc._h, good, n) == dg.DG_OK

    def three(W, H, v, p, st=None, ps=None):
        """The three host entries' return codes, which must agree; a refused call writes nothing."""
        img[:] = 0
        a = L.dg_map_thing_lines(sc._h, W, H, ctypes.byref(v), ctypes.byref(p), st, ps, None, 0)
        b = L.dg_ego_map_things_host(sc._h, W, H, ctypes.byref(v), ctypes.byref(p), None, st, ps, P(img))
        assert b == dg.DG_OK or not img.any()
        e = L.dg_floor_map_things_host(sc._h, W, H, ctypes.byref(v), ctypes.byref(p), None, st, None, ps, P(img))
        assert (a < 0) == (b < 0) == (e < 0) and (a >= 0 or a == b == e) and (e == dg.DG_OK or not img.any())
        return b

    assert three(64, 48, v, p) == dg.DG_OK and img.any()
    for W, H in ((15, 48), (64, 15), (16385, 48), (0, 48)):
        assert three(W, H, v, p) == dg.DG_ERR_INVALID
    for scale, flags in ((0.0, 0), (64.5, 0), (float("nan"), 0), (1.0, 4)):
        assert three(64, 48, v, dg.DgEgoMap(scale, flags)) == dg.DG_ERR_INVALID
    for bad in (65537.0, float("nan"), float("inf")):
        assert three(64, 48, dg.DgView(bad, 0.0, 0.5, 0, 0, 0, 0, 0, 0, 0), p) == dg.DG_ERR_INVALID
    assert three(64, 48, dg.DgView(0.0, 0.0, 0.5, 0, 1.5, 0.0, 0, 0, 0, 1), p) == dg.DG_ERR_INVALID
    # pose and state entries, validated as the view submissions validate them
    for entries in ([(n, 0.0, 0.0, 0.0)], [(-1, 0.0, 0.0, 0.0)], [(0, 1.0, 1.0, 0.0), (n + 5, 0.0, 0.0, 0.0)]):
        ps, _k = dg.make_view_poses([entries])
        assert three(64, 48, v, p, None, ps) == dg.DG_ERR_INVALID
    assert three(64, 48, v, p, None, (dg.DgViewPoses * 1)(dg.DgViewPoses(None, 2))) == dg.DG_ERR_INVALID
    for lights, mobjs in (([], [(n, 0, 0)]), ([], [(-1, 0, 0)]), ([], [(0, 1 << 20, 0)]), ([(99, 100)], [])):
        st, _k = dg.make_view_states([(lights, mobjs)])
        assert three(64, 48, v, p, st) == dg.DG_ERR_INVALID
    assert three(64, 48, v, p, (dg.DgViewState * 1)(dg.DgViewState(None, 0, None, 1))) == dg.DG_ERR_INVALID
    ok_ps, _k = dg.make_view_poses([[(0, 1.0, 1.0, float("nan")), (n - 1, float("inf"), 0.0, 0.0)]])       # the floats are taken as given
    assert three(64, 48, v, p, None, ok_ps) == dg.DG_OK
    # NULL arguments
    assert L.dg_map_thing_lines(None, 64, 48, bv, bp, None, None, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_map_thing_lines(sc._h, 64, 48, None, bp, None, None, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_map_thing_lines(sc._h, 64, 48, bv, None, None, None, None, 0) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_things_host(None, 64, 48, bv, bp, None, None, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_ego_map_things_host(sc._h, 64, 48, bv, bp, None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_floor_map_things_host(None, 64, 48, bv, bp, None, None, None, None, P(img)) == dg.DG_ERR_INVALID
    assert L.dg_floor_map_things_host(sc._h, 64, 48, bv, bp, None, None, None, None, None) == dg.DG_ERR_INVALID
    # cap too small: the count comes back and nothing is written
    arr = (dg.DgMapLine * count)()
    assert L.dg_map_thing_lines(sc._h, 64, 48, bv, bp, None, None, arr, count - 1) == count and not any(bytes(arr))
    assert L.dg_map_thing_lines(sc._h, 64, 48, bv, bp, None, None, arr, count) == count and any(bytes(arr))
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    assert L.dg_submit_ego_map_views_things(None, 0, bv, 1, bp, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_render_ego_map_views_things(None, bv, 1, bp, None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_submit_floor_map_views_things(None, 0, bv, 1, bp, None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_render_floor_map_views_things(None, bv, 1, bp, None, None, None, None, None) == dg.DG_ERR_INVALID


def test_more_than_65536_map_objects_is_a_capacity_error(dg, synth):
    """A THINGS lump of 65 537 map objects behind the hand world's start: DG_ERR_CAPACITY at every thing call; 65 536 are drawn."""
    import struct
    base = fc.wad_of("hand")
    for n_obj, want_ok in ((65537, False), (65536, True)):
        lumps = mf._lumps(base)
        i = next(k for k, (nm, _) in enumerate(lumps) if nm == "THINGS")
        start = lumps[i][1][:10]
        lumps[i] = ("THINGS", start + b"".join(struct.pack("<hhhhh", 100 + k % 500, 150 + (k // 500) % 200, (k * 45) % 360, 2035, 7) for k in range(n_obj)))
        sc = dg.Scene(mf._pack(lumps), "e1m1")
        assert sc.mobj_count() == n_obj
        L = dg.lib()
        v, p = dg.DgView(352.5, 250.0, 0.1, 0, 0, 0, 0, 0, 0, 0), dg.DgEgoMap(0.05, 3)
        img = np.zeros((16, 16, 3), np.uint8)
        a = L.dg_map_thing_lines(sc._h, 16, 16, ctypes.byref(v), ctypes.byref(p), None, None, None, 0)
        b = L.dg_ego_map_things_host(sc._h, 16, 16, ctypes.byref(v), ctypes.byref(p), None, None, None, img.ctypes.data_as(dg._P))
        e = L.dg_floor_map_things_host(sc._h, 16, 16, ctypes.byref(v), ctypes.byref(p), None, None, None, None, img.ctypes.data_as(dg._P))
        assert (a, b, e) == ((0, dg.DG_OK, dg.DG_OK) if want_ok else (dg.DG_ERR_CAPACITY,) * 3)
        if want_ok:
            sc.set_map_markers([(4, 0x00ff00, 1)] * n_obj)
            assert L.dg_map_thing_lines(sc._h, 16, 16, ctypes.byref(v), ctypes.byref(p), None, None, None, 0) == 4 * n_obj
        sc.close()


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_scene_set_map_markers", "dg_map_thing_lines", "dg_ego_map_things_host", "dg_floor_map_things_host", "dg_submit_ego_map_views_things",
             "dg_render_ego_map_views_things", "dg_submit_floor_map_views_things", "dg_render_floor_map_views_things"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert (dg.DG_MARK_BOX, dg.DG_MARK_HEADING) == (1, 2) and ctypes.sizeof(dg.DgMapMarker) == 12
    assert dg.lib().dg_version() == b"doomgpu 0.6 (gfx950; ABI 4)"
    for f in (dg.map_thing_lines, dg.ego_map_things_host, dg.floor_map_things_host, dg.Scene.set_map_markers, dg.Context.submit_ego_map_things,
              dg.Context.render_ego_map_things, dg.Context.submit_floor_map_things, dg.Context.render_floor_map_things):
        assert callable(f)
    header = open(dg.INCLUDE).read()
    assert "typedef struct dg_map_marker { int32_t radius; uint32_t rgb; uint32_t flags; } dg_map_marker;" in header
    assert "enum { DG_MARK_BOX = 1u, DG_MARK_HEADING = 2u };" in header


def test_the_things_phase_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/map_things/map_things_host_main.cpp (its own main) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: the kernels' things phase as a host loop over the shared inline functions, for
    every band height, against dg_ego_map_things_host; the host entries with buffers of exactly the contract's sizes.  It checks its own
    results; any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "map_things_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "map_things", "map_things_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "light.wad"
    wad.write_bytes(fc.wad_of("light"))
    r = subprocess.run([str(exe), str(wad), "e1m1"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "map_things_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
