"""GPU tier of the map-object markers on the map frames: dg_ego_thing_tiles and dg_floor_thing_tiles against
dg_ego_map_things_host / dg_floor_map_things_host, byte for byte — the host entries are held against the numpy restatement by
tests/test_map_things_host.py.

   64x48     one band, 16-byte stores                   333x77    byte stores, four bands of 24 rows (the last of 5)
   1280x800  6-row bands, three frames                  8200x16   the wide tile: one row per band, one frame
Every size runs cases of map_thing_cases.py as a submission whose frames move the view, with the case's poses and states in the first and
the last frame; further down: batches of 1, 9 and max_batch, the doom2-scale map (2 500 items: ten chunks a band), a box across a band
boundary, an object moved across the frame over nine frames, objects hidden by state, masks and arrows, no table, replay, a second
upload, a 3-D submission in the other slot, and the error returns.
"""
import ctypes

import numpy as np
import pytest

import floor_map_cases as fc
import map_thing_cases as mc

pytestmark = pytest.mark.gpu

NAMES = ("hand_whole_2", "hand_whole_3", "hand_unit", "light_near_7", "light_near_33", "later_pose_wins", "state_entry_hides", "heading_not_finite", "radius_0",
         "over_a_line_under_the_arrow", "at_the_player", "black_marker", "pose_at_32768")


@pytest.fixture(scope="module")
def scenes(dg):
    out = {w: fc.open_scene(dg, w) for w in ("light", "hand")}
    yield out
    for sc in out.values():
        sc.close()


def _batch(dg, c, n):
    """n frames of case c: (views, mask rows or None, states or None, poses or None) as lists per frame."""
    views = (dg.DgView * n)()
    x, y, a = c["view"]
    for k in range(n):
        views[k] = dg.DgView(x + 3.5 * k, y - 1.25 * k, a + 0.05 * k, 0, 0, 0, 0, 0, c["ts"] + 0.35 * k, 0)
    masks = None if c["mask"] is None else np.stack([fc.mask_row(c, k) for k in range(n)])
    with_entries = lambda k: k == 0 or k == n - 1
    states = None if not c["mobjs"] else [mc.state_of(c) if with_entries(k) else ([], []) for k in range(n)]
    poses = None if not c["poses"] else [mc.poses_of(c) if with_entries(k) else [] for k in range(n)]
    return views, masks, states, poses


def _host(dg, sc, W, H, c, batch, floor):
    views, masks, states, poses = batch
    out = []
    for k in range(len(views)):
        m, st, ps = (None if masks is None else masks[k]), (None if states is None else states[k]), (None if poses is None else poses[k])
        p = (c["scale"], c["flags"])
        out.append(dg.floor_map_things_host(sc, W, H, views[k], p, m, st, None, ps) if floor else dg.ego_map_things_host(sc, W, H, views[k], p, m, st, ps))
    return np.stack(out)


def _check_case(dg, ctx, sc, c, W, H, n, kinds=(False, True)):
    """Case c as n frames through both kernels; returns the host's ego frames."""
    batch = _batch(dg, c, n)
    views, masks, states, poses = batch
    p = (c["scale"], c["flags"])
    for floor in kinds:
        got = ctx.render_floor_map_things(views, p, masks, states, None, poses) if floor else ctx.render_ego_map_things(views, p, masks, states, poses)
        want = _host(dg, sc, W, H, c, batch, floor)
        for f in range(n):
            assert np.array_equal(got[f], want[f]), (c["name"], "floor" if floor else "ego", W, H, f, int((got[f] != want[f]).any(axis=2).sum()))
    return want


def _check_world(dg, scenes, world, W, H, n, names, kinds=(False, True)):
    sc = scenes[world]
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    for name in names:
        c = mc.BY_NAME[name]
        if c["world"] != world:
            continue
        sc.set_map_markers(mc.table(world, c["marked"]))
        ctx.upload_scene(sc)                                                   # (the ctx takes the marker table here)
        _check_case(dg, ctx, sc, c, W, H, n, kinds)
        if c["shown"] and name != "black_marker" and (W, H) == (64, 48):            # the markers are in the frame: the case cannot pass without them
            v, p = fc.view_of(dg, c), (c["scale"], c["flags"])
            assert not np.array_equal(dg.ego_map_things_host(sc, W, H, v, p, fc.mask_row(c), mc.state_of(c), mc.poses_of(c)), dg.ego_map_host(sc, W, H, v, p, fc.mask_row(c))), name
    ctx.close()


@pytest.mark.parametrize("world", ["light", "hand"])
@pytest.mark.parametrize("size", [(64, 48), (333, 77)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_host_rule(dg, scenes, size, world):
    _check_world(dg, scenes, world, *size, 3, NAMES)


def test_three_frames_at_1280x800(dg, scenes):
    """Bands of 6 rows: every box taller than that lies across band boundaries."""
    _check_world(dg, scenes, "light", 1280, 800, 3, ("light_near_7",))
    _check_world(dg, scenes, "hand", 1280, 800, 3, ("hand_unit", "over_a_line_under_the_arrow"), kinds=(False,))


def test_one_frame_on_the_wide_tile(dg, scenes):
    _check_world(dg, scenes, "hand", 8200, 16, 1, ("hand_whole_3", "at_the_player"))


def test_batches_of_1_9_and_max_batch(dg, scenes):
    W, H, F = 64, 48, 24
    sc = scenes["light"]
    sc.set_map_markers(mc.default_table("light"))
    ctx = dg.Context(W, H, max_batch=F, slots=1)
    ctx.upload_scene(sc)
    for n in (1, 9, F):
        for name in ("light_near_0", "light_near_19"):
            c = dict(mc.BY_NAME[name], scale=0.25)
            _check_case(dg, ctx, sc, c, W, H, n)
    ctx.close()


def test_the_doom2_scale_map_takes_ten_chunks_a_band(dg, synth):
    """500 map objects, all marked with box and heading: 2 500 items, ten chunks of EGO_CHUNK per band, most of the level in the frame —
    several hundred marker lines survive, so a band's survivors come from several chunks."""
    wad = synth.build_synth_iwad(2002, heavy=True, vanilla=True, grid=(32, 24), n_things=500)
    sc = dg.Scene(wad, "e1m1")
    n = sc.mobj_count()
    assert n * 5 > 9 * 256
    sc.set_map_markers([(16 + 16 * (i % 4), mc.rgb_of(i), 3) for i in range(n)])
    placed = sc.mobj_poses()
    cx, cy = float(np.median(placed["x"])), float(np.median(placed["y"]))
    W, H = 333, 77
    ctx = dg.Context(W, H, max_batch=3, slots=1)
    ctx.upload_scene(sc)
    for scale, flags in ((0.02, fc.A), (0.01, fc.R | fc.A)):
        views = (dg.DgView * 3)(*[dg.DgView(cx + 40.0 * k, cy - 25.0 * k, 0.4 * k, 0, 0, 0, 0, 0, 0, 0) for k in range(3)])
        poses = [[], [(i, float(placed["x"][i]) + 30.0, float(placed["y"][i]) - 30.0, 0.1 * i) for i in range(0, n, 3)], [(n - 1, cx, cy, 1.0)]]
        got = ctx.render_ego_map_things(views, (scale, flags), None, None, poses)
        for k in range(3):
            want = dg.ego_map_things_host(sc, W, H, views[k], (scale, flags), None, None, poses[k])
            assert np.array_equal(got[k], want), (scale, k, int((got[k] != want).any(axis=2).sum()))
            lines = dg.map_thing_lines(sc, W, H, views[k], (scale, flags), None, poses[k])
            in_frame = sum(1 for x0, y0, x1, y1, _ in lines.tolist() if max(x0, x1) >= 0 and min(x0, x1) < W and max(y0, y1) >= 0 and min(y0, y1) < H)
            assert len(lines) == 5 * n and in_frame > 256, (scale, k, in_frame)              # more survivors than one chunk holds
        got = ctx.render_floor_map_things(views, (scale, flags), None, None, None, poses)
        assert np.array_equal(got[1], dg.floor_map_things_host(sc, W, H, views[1], (scale, flags), None, None, None, poses[1]))
    ctx.close()
    sc.close()


def test_a_box_across_a_band_boundary_and_an_object_moved_across_the_frame(dg, scenes):
    """333x77: bands of 24 rows.  The imp's box (radius 10 at scale 1) is put on rows 14 .. 34, across the boundary at row 24; then nine
    frames move it from the left edge to the right edge, each frame with a pose of its own."""
    W, H, n = 333, 77, 9
    sc = scenes["hand"]
    sc.set_map_markers(mc.table("hand", {0: (10, mc.rgb_of(0), 3)}))
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(sc)
    v = dg.DgView(600.0, 236.0, 0.0, 0, 0, 0, 0, 0, 0, 0)                           # the imp at (600, 250): Y = 38 - 14 = 24
    lines = dg.map_thing_lines(sc, W, H, v, (1.0, 0))
    assert min(l[1] for l in lines.tolist()) == 14 and max(l[1] for l in lines.tolist()) == 34
    got = ctx.render_ego_map_things((dg.DgView * 1)(v), (1.0, 0))
    assert np.array_equal(got[0], dg.ego_map_things_host(sc, W, H, v, (1.0, 0)))
    rgb = mc.rgb_of(0)
    marker = lambda frame: (frame == [rgb & 255, (rgb >> 8) & 255, rgb >> 16]).all(axis=2)
    assert marker(got[0])[14:24].any() and marker(got[0])[24:35].any()
    views = (dg.DgView * n)(*[v] * n)
    poses = [[(0, 600.0 - 160.0 + 40.0 * k, 250.0 + 2.0 * k, 0.3 * k)] for k in range(n)]
    for floor in (False, True):
        got = ctx.render_floor_map_things(views, (1.0, fc.A), None, None, None, poses) if floor else ctx.render_ego_map_things(views, (1.0, fc.A), None, None, poses)
        cols = []
        for k in range(n):
            want = dg.floor_map_things_host(sc, W, H, v, (1.0, fc.A), None, None, None, poses[k]) if floor else dg.ego_map_things_host(sc, W, H, v, (1.0, fc.A), None, None, poses[k])
            assert np.array_equal(got[k], want), (floor, k)
            if not floor:
                cols.append(int(np.nonzero(marker(got[k]).any(axis=0))[0].mean()))
        assert floor or (cols == sorted(cols) and cols[0] < 30 and cols[-1] > W - 30)        # left to right across the frame
    ctx.close()


def test_hidden_by_state_masks_and_arrows(dg, scenes):
    W, H, n = 64, 48, 4
    sc = scenes["hand"]
    c = mc.BY_NAME["hand_whole_0"]
    sc.set_map_markers(mc.table("hand", c["marked"]))
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    ctx.upload_scene(sc)
    views = (dg.DgView * n)(*[fc.view_of(dg, c)] * n)
    states = [([], []), ([], [(0, -1, 0)]), ([], [(0, -1, 0), (1, -1, 0), (2, -1, 0)]), ([], [(0, -1, 0), (0, 0, 0)])]
    ones = fc.model_of("hand").ego.bits_to_row(range(fc.model_of("hand").ego.n_lines))
    for flags in (0, fc.R, fc.A, fc.R | fc.A):
        for mask in (None, np.stack([ones, ones & 5, ones * 0, ones])):
            p = (c["scale"], flags)
            got = ctx.render_ego_map_things(views, p, mask, states)
            want = [dg.ego_map_things_host(sc, W, H, views[k], p, None if mask is None else mask[k], states[k]) for k in range(n)]
            plain = dg.ego_map_host(sc, W, H, views[2], p, None if mask is None else mask[2])
            assert all(np.array_equal(got[k], want[k]) for k in range(n)), (flags, mask is None)
            assert np.array_equal(got[2], plain) and not np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[3])
            gotf = ctx.render_floor_map_things(views, p, mask, states)
            assert all(np.array_equal(gotf[k], dg.floor_map_things_host(sc, W, H, views[k], p, None if mask is None else mask[k], states[k])) for k in range(n))
    ctx.close()


def test_no_table_equals_the_plain_submission_and_a_second_upload_takes_another_table(dg, scenes):
    W, H, n = 320, 200, 3
    sc = scenes["light"]
    c = dict(mc.BY_NAME["light_near_7"], scale=0.25)
    batch = _batch(dg, c, n)
    views, masks, _, _ = batch
    p = (c["scale"], c["flags"])
    ctx = dg.Context(W, H, max_batch=n, slots=1)
    sc.set_map_markers(None)
    ctx.upload_scene(sc)
    plain_ego, plain_floor = ctx.render_ego_map(views, p, masks), ctx.render_floor_map(views, p, masks)
    assert np.array_equal(ctx.render_ego_map_things(views, p, masks), plain_ego) and np.array_equal(ctx.render_floor_map_things(views, p, masks), plain_floor)
    first = None
    for table in (mc.default_table("light"), [(r + 4, rgb ^ 0x4000, 3) for r, rgb, _ in mc.default_table("light")], [(16, 0x808080, 0)] * sc.mobj_count()):
        sc.set_map_markers(table)
        if first is not None:                                                  # set on the scene, not uploaded yet: the ctx draws with the table it took
            assert np.array_equal(ctx.render_ego_map_things(views, p, masks), first)
        ctx.upload_scene(sc)
        got = ctx.render_ego_map_things(views, p, masks)
        assert np.array_equal(got, _host(dg, sc, W, H, c, batch, False))
        assert np.array_equal(ctx.render_floor_map_things(views, p, masks), _host(dg, sc, W, H, c, batch, True))
        assert first is None or not np.array_equal(got, first)
        first = got
    assert np.array_equal(first, plain_ego)                                    # all flags 0: the plain frames
    ctx.close()


def test_timing_replay_and_readbacks(dg, scenes):
    W, H, n = 320, 200, 6
    sc = scenes["light"]
    sc.set_map_markers(mc.default_table("light"))
    c = dict(mc.BY_NAME["light_near_19"], scale=0.25, flags=fc.R | fc.A, mask=("half", 3))
    ctx = dg.Context(W, H, max_batch=8, slots=2)
    ctx.upload_scene(sc)
    batch = _batch(dg, c, n)
    views, masks, _, _ = batch
    n_obj = sc.mobj_count()
    poses = [[(i, 300.0 + 17.0 * i + 5.0 * k, 260.0 + 11.0 * i, 0.2 * k) for i in range(k % n_obj, n_obj, 3)] for k in range(n)]
    states = [([], [(k, -1, 0)]) for k in range(n)]
    batch = (views, masks, states, poses)
    p = (c["scale"], c["flags"])
    for floor, fe in ((False, dg.DG_FE_MAP_EGO), (True, dg.DG_FE_MAP_FLOOR)):
        want = _host(dg, sc, W, H, c, batch, floor)
        sent = np.array(masks)
        if floor:
            ctx.submit_floor_map_things(1, views, p, sent, states, None, poses)
        else:
            ctx.submit_ego_map_things(1, views, p, sent, states, poses)
        sent[:] = 0xFFFFFFFF                                                   # the call copied what it needs
        assert np.array_equal(ctx.readback(1, 0, n), want)
        t = ctx.timing(1)
        assert t["front_end"] == fe and t["n_frames"] == n and t["raster_ms"] > 0
        sums = list(ctx.frame_checksums(1, 0, n))
        assert sums == [dg.frame_checksum(w) for w in want]
        ctx.submit_ego_map(0, views, (1.0, 0))                                  # a plain submission in the other slot in between
        ctx.wait(0)
        ctx.replay(1)
        ctx.wait(1)
        t = ctx.timing(1)
        assert t["front_end"] == fe and t["setup_ms"] == 0.0 and t["raster_ms"] > 0
        assert list(ctx.frame_checksums(1, 0, n)) == sums and np.array_equal(ctx.readback(1, 0, n), want)
        assert np.array_equal(ctx.readback_reduced(1, 0, n, (4, 4)), dg.reduce_host(want, (4, 4)))
        # a submission with fewer entries, then one with more than any before: the slot's block grows
        assert np.array_equal(ctx.render_ego_map_things(views, p, masks), _host(dg, sc, W, H, c, (views, masks, None, None), False))
        more = [[(i, 300.0 + 3.0 * i, 250.0 + k, 0.0) for i in range(n_obj)] * 3 for k in range(n)]
        assert np.array_equal(ctx.render_ego_map_things(views, p, masks, None, more), _host(dg, sc, W, H, c, (views, masks, None, more), False))
    ctx.close()


def test_a_things_submission_and_a_3d_submission_in_flight(dg, oracle, wad1993, path1993):
    W, H = 320, 200
    sc = dg.Scene(wad1993, "e1m1")
    sc.set_map_markers([(16, mc.rgb_of(i), 3) for i in range(sc.mobj_count())])
    osc = oracle.Scene(wad1993, "e1m1")
    recs = path1993[[0, 100, 297, 323, 500, 623, 728, 900]]
    v = dg.make_views(recs)
    p = (0.25, fc.R | fc.A)
    poses = [[(k, float(recs[k][0]) + 20.0, float(recs[k][1]), 0.5)] for k in range(8)]
    want3d = [dg.frame_checksum(osc.render(W, H, r)) for r in recs]
    wantmap = [dg.frame_checksum(dg.ego_map_things_host(sc, W, H, v[k], p, None, None, poses[k])) for k in range(8)]
    wantfloor = [dg.frame_checksum(dg.floor_map_things_host(sc, W, H, v[k], p, None, None, None, poses[k])) for k in range(8)]
    ctx = dg.Context(W, H, max_batch=8, slots=2)
    ctx.upload_scene(sc)
    for first, second in (("3d", "map"), ("map", "3d")):
        for slot, what in enumerate((first, second)):
            ctx.submit(slot, v) if what == "3d" else ctx.submit_ego_map_things(slot, v, p, None, None, poses)
        ctx.wait(0)
        ctx.wait(1)
        a, b = list(ctx.frame_checksums(0, 0, 8)), list(ctx.frame_checksums(1, 0, 8))
        assert (a, b) == ((want3d, wantmap) if first == "3d" else (wantmap, want3d))
    ctx.submit(0, v)
    ctx.submit_floor_map_things(1, v, p, None, None, None, poses)
    assert list(ctx.frame_checksums(1, 0, 8)) == wantfloor and list(ctx.frame_checksums(0, 0, 8)) == want3d
    ctx.submit_ego_map(1, v, p)                                                 # one slot: things, plain, things
    assert ctx.timing(1)["front_end"] == dg.DG_FE_MAP_EGO and list(ctx.frame_checksums(1, 0, 8)) != wantmap
    ctx.submit_ego_map_things(1, v, p, None, None, poses)
    assert list(ctx.frame_checksums(1, 0, 8)) == wantmap
    ctx.close()
    sc.close()


def test_error_returns_through_the_ctx_leave_the_slot_as_it_was(dg, scenes):
    sc = scenes["hand"]
    n_obj = sc.mobj_count()
    sc.set_map_markers(mc.table("hand", mc.BY_NAME["hand_whole_0"]["marked"]))
    L = dg.lib()
    v = (dg.DgView * 4)(*[dg.DgView(352.5, 250.0, 0.5, 0, 0, 0, 0, 0, 0, 0)] * 4)
    good = dg.DgEgoMap(0.05, fc.R | fc.A)
    g = ctypes.byref(good)
    ctx = dg.Context(320, 200, max_batch=3, slots=1)
    ego = lambda *a: L.dg_submit_ego_map_views_things(ctx._h, *a)
    floor = lambda slot, views, n, p, mask, st, ps: L.dg_submit_floor_map_views_things(ctx._h, slot, views, n, p, mask, st, None, ps)
    assert ego(0, v, 1, g, None, None, None) == dg.DG_ERR_INVALID and floor(0, v, 1, g, None, None, None) == dg.DG_ERR_INVALID     # no scene uploaded
    ctx.upload_scene(sc)
    for sub, fe, render in ((ego, dg.DG_FE_MAP_EGO, ctx.render_ego_map_things), (floor, dg.DG_FE_MAP_FLOOR, ctx.render_floor_map_things)):
        keep = render((dg.DgView * 3)(*v[:3]), good)
        sums = list(ctx.frame_checksums(0, 0, 3))

        def refused(rc, want=dg.DG_ERR_INVALID):                               # ... and the slot holds what it held
            assert rc == want and list(ctx.frame_checksums(0, 0, 3)) == sums and ctx.timing(0)["front_end"] == fe, rc

        refused(sub(0, v, 4, g, None, None, None), dg.DG_ERR_CAPACITY)
        refused(sub(0, v, 0, g, None, None, None), dg.DG_ERR_CAPACITY)
        assert sub(1, v, 1, g, None, None, None) == dg.DG_ERR_INVALID             # slot out of range
        refused(sub(0, None, 1, g, None, None, None))
        refused(sub(0, v, 1, None, None, None, None))
        for bad in (dg.DgEgoMap(0.0, 0), dg.DgEgoMap(65.0, 0), dg.DgEgoMap(1.0, 4)):
            refused(sub(0, v, 1, ctypes.byref(bad), None, None, None))
        mixed = (dg.DgView * 3)(v[0], v[1], dg.DgView(1e6, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
        refused(sub(0, mixed, 3, g, None, None, None))
        assert b"frame 2" in L.dg_last_error()
        ps, _k1 = dg.make_view_poses([[(0, 1.0, 2.0, 0.0)], [], [(1, 0.0, 0.0, 0.0), (n_obj, 0.0, 0.0, 0.0)]])
        refused(sub(0, v, 3, g, None, None, ps))
        assert b"frame 2" in L.dg_last_error()
        refused(sub(0, v, 3, g, None, None, (dg.DgViewPoses * 3)(dg.DgViewPoses(None, 0), dg.DgViewPoses(None, 1), dg.DgViewPoses(None, 0))))
        st, _k2 = dg.make_view_states([([], []), ([], [(n_obj, 0, 0)]), ([], [])])
        refused(sub(0, v, 3, g, None, st, None))
        assert b"frame 1" in L.dg_last_error()
        st, _k3 = dg.make_view_states([([], [(0, 1 << 20, 0)]), ([], []), ([], [])])
        refused(sub(0, v, 3, g, None, st, None))
        refused(sub(0, v, 3, g, None, (dg.DgViewState * 3)(dg.DgViewState(None, 0, None, 0), dg.DgViewState(None, 0, None, 2), dg.DgViewState(None, 0, None, 0)), None))
        assert np.array_equal(ctx.readback(0, 0, 3), keep)
        assert np.array_equal(render((dg.DgView * 3)(*v[:3]), good), keep)        # still usable
    ctx.close()
