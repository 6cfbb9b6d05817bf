"""Per-view surfaces on the GPU (include/doomgpu.h: dg_view_surfaces).  Everything is byte-exact.

  flat rows   the rows the row kernels write for the seg walk (dg_slot_sector_flats) equal the scene's flats with the entries applied:
              batches of 1, 3, 64 and 65 frames, entry totals 0, 1, 255, 256, 257 and every cell, a losing earlier entry for every fifth
  side table  frames without entries between frames that have them; one frame holding every entry of the batch; a batch of exactly
              64 x max_batch entries; a batch of one more, which falls back, is counted and gives the same pixels
  pixels      70 views — the named cases, then one to five visible sidedefs and sectors changed per view, with light, state, pose and
              height entries on top — through every front end against the oracle's frames of the per-view patched WADs
  wall fx     the same batch with the wall effect flags on, through the fx pair, against the oracle; and 24 views of the effects test WAD
              with overrides into live lists and onto scrolling sidedefs, against the oracle's frames of the baked per-view WADs
  dense       64 views with every sector's flats and a third of the sidedefs redrawn, through the seg walk and DG_FE_AUTO
  bundle      colour, depth and labels from one submission; the label plane's holes follow GRATE1
  redone      frames redone on the host after a column overflow keep their surfaces
              ... and read only the slot's copy: the caller's entry arrays are overwritten before dg_wait
  replay      dg_replay_slot of a batch with entries reproduces it; a slot reused after a scene with another sidedef count
  mirror      doomgpu.hpp with a sidedef and a sector changed between two render() calls
The scene is of a WAD with a texture and a flat no map uses (surface_cases.with_extras): dg_scene_use_texture / dg_scene_use_flat
decode and append them before the upload.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mobj_pose_cases as mp
import sector_height_cases as sh
import staging_cases
import surface_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [(320, 200), (131, 67)]
N_PIXELS = 70
FE_NAMES = {1: "host", 2: "device", 3: "device_segs", 0: "auto"}
STATE_SPRITES = [("TROO", 0), ("BAR1", 0), ("CAND", 0)]
ALL_TEXTURES = ["BRICK1", "BRICK2", "BRICK3", "PANEL1", "PANEL2", "WIDE1", "WIDE2", "TALL72", "COMBO1", "COMBO2", "STONE1", "STONE2", "METAL1", "METAL2", "HOLEY1",
                "GRATE1", "EXTRA1", "-"]
ALL_FLATS = ["FLOOR0", "FLOOR1", "FLOOR2", "FLOOR3", "FLOOR4", "FLOOR5", "CEIL0", "CEIL1", "CEIL2", "CEIL3", "NUKAGE1", "NUKAGE2", "NUKAGE3", "F_SKY1", "EXTRAFL"]


def dg_fe(dg, fe):
    return {0: dg.DG_FE_AUTO, 1: dg.DG_FE_HOST, 2: dg.DG_FE_DEVICE, 3: dg.DG_FE_DEVICE_SEGS}[fe]


@pytest.fixture(scope="module")
def wad(wad1993):
    return sc.with_extras(wad1993)


@pytest.fixture(scope="module")
def scene(dg, wad):
    s = dg.Scene(wad, "e1m1")
    for sprite, frame in STATE_SPRITES:
        s.sprite_frame(sprite, frame)                         # (decoded before any upload)
    return s


@pytest.fixture(scope="module")
def names(scene, wad):
    """Every name the tests use, asked before any upload; EXTRA1 and EXTRAFL are appended by it."""
    n = sc.Names(scene)
    used = set(scene.sidedef_surfaces()[:, 1:4].ravel())
    for t in ALL_TEXTURES + [t.lower() for t in sc.texture_names(wad) if not t.upper().startswith("SKY")]:
        n.texture(t)
    for f in ALL_FLATS + sc.flat_names(wad):
        n.flat_handle(f)
    for e in sc.loaded_sides(wad):
        for t in e[:3]:
            n.texture(t)
    for e in sc.loaded_flats(wad):
        for f in e:
            n.flat_handle(f)
    assert n.texture("EXTRA1") not in used and n.texture("EXTRA1") >= 0
    return n


def _assert_frames(got, want, what):
    for k in range(len(want)):
        bad = np.argwhere(np.any(got[k] != want[k], axis=2))
        assert len(bad) == 0, f"{what}: view {k}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"


def _flat_sets(rng, n_frames, n_sectors, total, handles):
    cells = rng.permutation(n_frames * n_sectors)[:total]
    views = [[] for _ in range(n_frames)]
    for j, c in enumerate(cells):
        f, s = int(c) // n_sectors, int(c) % n_sectors
        if j % 5 == 0:
            views[f].append((s, handles[0], handles[1]))      # (loses to the entry below)
        views[f].append((s, handles[int(rng.integers(len(handles)))], handles[int(rng.integers(len(handles)))]))
    return views


@pytest.mark.parametrize("n_frames", [1, 3, 64, 65])
def test_the_rows_the_flat_row_kernels_write(dg, scene, names, path1993, n_frames):
    W, H = SIZES[n_frames % 2]
    n_sectors = scene.sector_count()
    cells = n_frames * n_sectors
    base = scene.sector_flats()[:, 1:]
    handles = [names.flat_handle(f) for f in ALL_FLATS]
    ctx = dg.Context(W, H, max_batch=65, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    rng = np.random.default_rng(100 * n_frames)
    views = dg.make_views(path1993[[(7 * i + 3) % 1000 for i in range(n_frames)]])
    for total in sorted({t for t in (0, 1, 255, 256, 257, cells) if t <= cells}):
        sets = _flat_sets(rng, n_frames, n_sectors, total, handles)
        want = np.repeat(base[None], n_frames, axis=0)
        for f, entries in enumerate(sets):
            for s, a, b in entries:
                want[f, s] = (a, b)
        vf, keep = dg.make_view_surfaces([([], e) for e in sets])
        before = ctx.fallbacks()
        ctx.submit_surfaces(0, views, vf)
        got = ctx.slot_sector_flats(0, 0, n_frames)
        assert got.shape == (n_frames, n_sectors, 2) and got.dtype == np.int32
        bad = np.argwhere(np.any(got != want, axis=2))
        assert len(bad) == 0, f"{(n_frames, total)}: {len(bad)} cells differ, first (frame, sector) {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before, (n_frames, total)
        if n_frames > 2:
            assert np.array_equal(ctx.slot_sector_flats(0, 1, n_frames - 2), got[1:n_frames - 1])
        assert ctx.surface_timing(0) > 0.0                    # (empty entry arrays still have the rows filled: surfaces != NULL)
        assert ctx.sector_height_timing(0) > 0.0              # ... and the height rows, which the surface-reading pair reads too
        plain = ctx.render(views)
        ctx.submit_surfaces(0, views, None)                   # no surfaces: neither kernel, the plain pair, the loaded flats
        assert ctx.surface_timing(0) == 0.0 and ctx.sector_height_timing(0) == 0.0
        assert np.array_equal(ctx.readback(0, 0, n_frames), plain)
        assert np.array_equal(ctx.slot_sector_flats(0, 0, n_frames), np.repeat(base[None], n_frames, axis=0))
        del keep
    ctx.close()


@pytest.mark.parametrize("n_frames", [1, 65])
def test_all_three_row_kinds_in_one_batch(dg, scene, names, wad, path1993, n_frames):
    """Poses, sector entries and surfaces in ONE seg-walk batch: the three kinds of per-view rows share one launch
    sequence and one start-event rule.  Each kind's rows equal its own expected-row builder byte for byte, each kind's kernels have a
    time, and the frames are the host walker's of the same batch; a batch without per-view inputs on the same slot then runs none of
    them, reads the scene's rows and is the host walker's again."""
    W, H = 131, 67
    n_mobjs = scene.mobj_count()
    rng = np.random.default_rng(8 + n_frames)
    pose_cases = mp.batch_cases(scene, wad, path1993, n_frames)
    dense = sc.random_cases(wad, n_frames, seed=77 + n_frames)
    cases = []
    for k in range(n_frames):
        f = pose_cases[k].frame
        sides = dense[k].sides
        sides = [sides[(j * len(sides)) // 64] for j in range(64)] if len(sides) > 64 else sides       # (the side table holds 64 per frame)
        cases.append(sc.Case(f"all{k}", f, sides, dense[k].flats, heights=sh.random_row(wad, rng, "jitter"), poses=pose_cases[k].entries,
                             timestamp=float(np.float32(0.25 * (k % 5)))))
    vf, keep0 = dg.make_view_surfaces([c.surfaces(names) for c in cases])
    vs, keep1 = dg.make_view_sectors([c.heights for c in cases])
    vp, keep2 = dg.make_view_poses([mp.entries_as_poses(c.poses) for c in cases])
    views = dg.make_views(np.stack([c.record(path1993)[:8] for c in cases]))
    for i, c in enumerate(cases):
        views[i].timestamp = c.timestamp
    base_poses = scene.mobj_poses()
    want_poses = np.tile(base_poses, (n_frames, 1))
    for k, c in enumerate(cases):
        for m, (x, y, deg) in mp.resolved(c.poses).items():
            px, py, ang = mp.pose(x, y, deg)
            want_poses[k, m] = (px, py, ang, int(scene.sectors_at([px], [py])[0]))
    want_heights = sh.expected_rows(wad, [sh.Case("", 0, c.heights) for c in cases])
    want_flats = sc.expected_flat_rows(scene, names, cases)
    base_heights, base_flats = sh.loaded_heights(wad), scene.sector_flats()[:, 1:]

    def bits(rows):
        return np.ascontiguousarray(rows).view(np.uint8)
    host = dg.Context(W, H, max_batch=65, slots=1, front_end=dg_fe(dg, 1))
    host.upload_scene(scene)
    host.submit_surfaces(0, views, vf, poses=vp, sectors=vs)
    host_sums = host.frame_checksums(0, 0, n_frames)
    host.submit_surfaces(0, views, None)
    host_plain = host.frame_checksums(0, 0, n_frames)
    host.close()
    assert not np.array_equal(host_sums, host_plain)

    ctx = dg.Context(W, H, max_batch=65, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    before = ctx.fallbacks()
    ctx.submit_surfaces(0, views, vf, poses=vp, sectors=vs)
    got_poses = ctx.slot_mobj_poses(0, 0, n_frames)
    assert got_poses.shape == (n_frames, n_mobjs) and np.array_equal(bits(got_poses), bits(want_poses))
    assert np.array_equal(bits(ctx.slot_sector_heights(0, 0, n_frames)), bits(want_heights))
    assert np.array_equal(bits(ctx.slot_sector_flats(0, 0, n_frames)), bits(want_flats))
    assert not np.array_equal(bits(want_poses), bits(np.tile(base_poses, (n_frames, 1)))) and not np.array_equal(want_heights[0], base_heights)
    assert not np.array_equal(want_flats[0], base_flats)
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before
    times = (ctx.mobj_pose_timing(0), ctx.sector_height_timing(0), ctx.surface_timing(0))
    print("all three kinds:", n_frames, "pose / height / flat kernels ms", times)
    assert all(np.isfinite(t) and t >= 0.0 for t in times), times
    assert np.array_equal(ctx.frame_checksums(0, 0, n_frames), host_sums)
    # the same slot without per-view inputs: none of the six kernels, the scene's rows, the plain frames
    ctx.submit_surfaces(0, views, None)
    assert (ctx.mobj_pose_timing(0), ctx.sector_height_timing(0), ctx.surface_timing(0)) == (0.0, 0.0, 0.0)
    assert np.array_equal(bits(ctx.slot_mobj_poses(0, 0, n_frames)), bits(np.tile(base_poses, (n_frames, 1))))
    assert np.array_equal(ctx.slot_sector_heights(0, 0, n_frames), np.repeat(base_heights[None], n_frames, axis=0))
    assert np.array_equal(ctx.slot_sector_flats(0, 0, n_frames), np.repeat(base_flats[None], n_frames, axis=0))
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before
    assert np.array_equal(ctx.frame_checksums(0, 0, n_frames), host_plain)
    ctx.close()
    del keep0, keep1, keep2


def test_the_side_table_at_its_shapes_and_its_capacity(dg, scene, names, wad, path1993, pixel_batch):
    """The reference is the host front end of the same scene and entries (equal to the oracle on the CPU tier and in the pixel tests)."""
    W, H = 131, 67
    n = 6
    cap = 64 * n
    sides = sc.loaded_sides(wad)
    n_sd = len(sides)
    assert n_sd > cap + 1
    rng = np.random.default_rng(9)
    tex = [t for t in ALL_TEXTURES if t not in ("-", "GRATE1")]

    def entry(i):
        return (i,) + tuple(names.texture(m if m == "-" else tex[int(rng.integers(len(tex)))]) for m in sides[i][:3]) + (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))
    ends = {c.name: c for c in pixel_batch["cases"] if c.name in ("first_sidedef", "last_sidedef")}      # (the lowest and highest sidedef with a seg, and a frame that sees each)
    lo, hi = ends["first_sidedef"].sides[0][0], ends["last_sidedef"].sides[0][0]
    f_lo, f_hi = ends["first_sidedef"].frame, ends["last_sidedef"].frame
    assert lo == min(sd for sd in sc.seg_sides(wad) if sd >= 0) and hi == max(sc.seg_sides(wad))
    views_std, views_ends = dg.make_views(path1993[[40, 114, 217, 323, 640, 817]]), dg.make_views(path1993[[f_lo, f_hi, 217, 323, f_hi, f_lo]])
    host = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, 1))
    host.upload_scene(scene)
    ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    plains = {False: host.render(views_std), True: host.render(views_ends)}
    order = [int(i) for i in rng.permutation(n_sd)]
    shapes = {
        "gaps": [[entry(i) for i in order[:50]], [], [], [entry(i) for i in order[50:51]], [], [entry(i) for i in order[:64]]],
        "one frame holds all": [[], [], [entry(i) for i in order[:cap]], [], [], []],
        "first and last sidedef": [[entry(lo), entry(hi)], [entry(hi)], [], [], [entry(lo), entry(hi)], [entry(hi), entry(lo)]],
        "exactly the capacity": [[entry(i) for i in order[k * 64:(k + 1) * 64]] for k in range(n)],
        "one more": [[entry(i) for i in order[k * 64:(k + 1) * 64 + (k == 3)]] for k in range(n)],
    }
    assert sum(len(v) for v in shapes["exactly the capacity"]) == cap and sum(len(v) for v in shapes["one more"]) == cap + 1
    for what, sets in shapes.items():
        sets = [list(reversed(s)) for s in sets]              # (unsorted, as a caller may give them)
        vf, keep = dg.make_view_surfaces([(s, []) for s in sets])
        views, plain = (views_ends, plains[True]) if what == "first and last sidedef" else (views_std, plains[False])
        want = host.render_surfaces(views, vf)
        before = ctx.fallbacks()
        got = ctx.render_surfaces(views, vf)
        _assert_frames(got, want, what)
        assert not np.array_equal(want, plain), what
        if what == "first and last sidedef":                  # each end of the span moves pixels in the frames that see it
            assert all(not np.array_equal(want[k], plain[k]) for k in (0, 1, 4, 5)) and all(np.array_equal(want[k], plain[k]) for k in (2, 3))
        after = ctx.fallbacks()
        if what == "one more":
            assert after["front_end"] == before["front_end"] + 1 and ctx.timing(0)["front_end"] != dg.DG_FE_DEVICE_SEGS and ctx.surface_timing(0) == 0.0
        else:
            assert after == before and ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.surface_timing(0) > 0.0, what
        del keep
    host.close()
    ctx.close()


def _view_state(v, n_sectors, n_mobjs):
    sprite, frame = STATE_SPRITES[v % len(STATE_SPRITES)]
    lights = [((v * 3) % n_sectors, 96 + (v * 16) % 160)]
    mobjs = [((v * 5 + 1) % n_mobjs, (sprite, frame), v % 2)] + ([((v * 5 + 2) % n_mobjs, None, 0)] if v % 3 == 0 else [])
    return lights, mobjs


@pytest.fixture(scope="module")
def pixel_batch(dg, oracle, scene, names, wad, path1993):
    """The 70 cases — the named ones first, then one to five visible sidedefs and sectors changed per view, with height and pose entries —
    with light and state entries on top, and per size the oracle's frames of the per-view patched WADs."""
    side_pairs, flat_pairs = sc.visible_pairs(oracle, wad, path1993)
    cases = sc.named_cases(scene, oracle, wad, path1993, side_pairs, flat_pairs, "EXTRA1", "EXTRAFL")
    sides, flats = sc.loaded_sides(wad), sc.loaded_flats(wad)
    hs = sh.loaded_heights(wad).astype(int)
    n_sectors, n_mobjs = scene.sector_count(), scene.mobj_count()
    sd_by, fl_by = {}, {}
    for f, i in side_pairs:
        sd_by.setdefault(f, []).append(i)
    for f, s in flat_pairs:
        fl_by.setdefault(f, []).append(s)
    frames = sorted(set(sd_by) & set(fl_by))
    tex = [t for t in ALL_TEXTURES if t != "-"]
    for v in range(len(cases), N_PIXELS):
        f = frames[(v * 3) % len(frames)]
        se, fe = [], []
        for j in range(v % 5 + 1):
            i = sd_by[f][(v + j) % len(sd_by[f])]
            m, l, u, x, y = sides[i]
            t = tex[(v + 3 * j) % len(tex)]
            se.append((i, t if (m != "-" or t == "GRATE1") else "-", l if l == "-" else t, u if u == "-" else t, x + v - 30, y - j))
            s = fl_by[f][(v + 2 * j) % len(fl_by[f])]
            fe.append((s, ALL_FLATS[(v + j) % len(ALL_FLATS)], ALL_FLATS[(2 * v + j) % len(ALL_FLATS)]))
        s0 = fe[0][0]
        heights = [(s0, hs[s0, 0] + 8, hs[s0, 1] - 8)] if v % 2 else []
        a = mp.ahead(path1993, f, 0)
        poses = [((v * 7) % n_mobjs,) + mp.target(path1993, f + a[v % len(a)]) + ((v * 29) % 360 - 180,)] if v % 2 == 0 and a else []
        cases.append(sc.Case(f"view{v}", f, se, fe, heights=heights, poses=poses, timestamp=float(np.float32(0.35 * (v % 7)))))
    st = [_view_state(v, n_sectors, n_mobjs) for v in range(N_PIXELS)]
    frames_of = {}

    def oracle_for(W, H):
        if (W, H) not in frames_of:
            out = np.empty((len(cases), H, W, 3), dtype=np.uint8)
            for k, c in enumerate(cases):
                def prepare(osc, k=k):
                    lights, mobjs = st[k]
                    for s, level in lights:
                        osc.set_sector_light(s, level)
                    for m, sp, fb in mobjs:
                        osc.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
                out[k] = sc.oracle_frame(oracle, c.patched(wad), c.record(path1993), W, H, prepare=prepare)
            frames_of[(W, H)] = out
        return frames_of[(W, H)]
    states = [(lights, [(m, scene.sprite_frame(*sp) if sp else -1, fb) for m, sp, fb in mobjs]) for lights, mobjs in st]
    for c in cases:                                           # (every name asked before any upload)
        c.surfaces(names)
    return {"cases": cases, "states": states, "named_states": st, "oracle": oracle_for}


def _batch(dg, path, names, pixel_batch, n):
    """The first n views of the pixel batch as the calls take them: (cases, views, surfaces, sectors, poses, states, keep-alive)."""
    cases = pixel_batch["cases"][:n]
    vf, keep0 = dg.make_view_surfaces([c.surfaces(names) for c in cases])
    vs, keep = dg.make_view_sectors([c.heights for c in cases])
    poses, keep2 = dg.make_view_poses([mp.entries_as_poses(c.poses) for c in cases])
    states, keep3 = dg.make_view_states(pixel_batch["states"][:n])
    views = dg.make_views(np.stack([c.record(path)[:8] for c in cases]))
    for i, c in enumerate(cases):
        views[i].timestamp = c.timestamp
    return cases, views, vf, vs, poses, states, (keep0, keep, keep2, keep3)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fe", [1, 2, 3, 0], ids=lambda f: FE_NAMES[f])
def test_pixels_equal_the_oracle_of_the_patched_wads(dg, scene, names, wad, path1993, pixel_batch, fe, size):
    W, H = size
    want = pixel_batch["oracle"](W, H)
    cases, views, vf, vs, poses, states, keep = _batch(dg, path1993, names, pixel_batch, N_PIXELS)
    assert [c.name for c in cases[:len(sc.NAMES)]] == sc.NAMES
    ctx = dg.Context(W, H, max_batch=N_PIXELS, slots=1, front_end=dg_fe(dg, fe))
    ctx.upload_scene(scene)
    before = ctx.fallbacks()
    got = ctx.render_surfaces(views, vf, states=states, poses=poses, sectors=vs)
    _assert_frames(got, want, (FE_NAMES[fe], size))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before
        assert ctx.surface_timing(0) > 0.0 and ctx.sector_height_timing(0) > 0.0 and ctx.mobj_pose_timing(0) > 0.0
    # the flats and heights every front end says it drew with
    assert np.array_equal(ctx.slot_sector_flats(0, 0, N_PIXELS), sc.expected_flat_rows(scene, names, cases)), FE_NAMES[fe]
    assert np.array_equal(ctx.slot_sector_heights(0, 0, N_PIXELS), sh.expected_rows(wad, [sh.Case("", 0, c.heights) for c in cases])), FE_NAMES[fe]
    # surfaces == NULL is dg_submit_views_sectors, byte for byte
    plain = ctx.render_sectors(views, vs, states=states, poses=poses)
    ctx.submit_surfaces(0, views, None, states=states, poses=poses, sectors=vs)
    assert np.array_equal(ctx.readback(0, 0, N_PIXELS), plain)
    assert ctx.surface_timing(0) == 0.0
    assert not np.array_equal(plain, got)
    ctx.close()
    del keep


def test_the_same_batch_with_the_wall_effects_on_goes_through_the_fx_pair(dg, wad, path1993, pixel_batch):
    """The pixel batch on a scene of the same WAD with both wall effect flags set: the seg walk of a batch with surfaces is then the
    surface-reading fx pair (dg_sfc_wfx_*; the launch asks only whether the flags are set).  This map has no live animation list and
    no special-48 linedef, so the frames are still the oracle's."""
    W, H = 131, 67
    want = pixel_batch["oracle"](W, H)
    s = dg.Scene(wad, "e1m1")
    for sprite, frame in STATE_SPRITES:
        s.sprite_frame(sprite, frame)
    nm = sc.Names(s)
    for c in pixel_batch["cases"]:
        c.surfaces(nm)
    s.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
    cases, views, vf, vs, poses, _, keep = _batch(dg, path1993, nm, pixel_batch, N_PIXELS)
    states, keep2 = dg.make_view_states([(lights, [(m, s.sprite_frame(*sp) if sp else -1, fb) for m, sp, fb in mobjs]) for lights, mobjs in pixel_batch["named_states"]])
    ctx = dg.Context(W, H, max_batch=N_PIXELS, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(s)
    before = ctx.fallbacks()
    got = ctx.render_surfaces(views, vf, states=states, poses=poses, sectors=vs)
    _assert_frames(got, want, "wall effects on, the pixel batch")
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before and ctx.surface_timing(0) > 0.0
    ctx.close()
    s.close()
    del keep, keep2


def test_overrides_under_live_wall_effects_equal_the_oracle_of_the_baked_wads(dg, oracle, path1993):
    """The effects test WAD (live animation lists, special-48 linedefs) with the effects on, 24 views of their own: overrides into live
    lists, into a list that is not live and onto scrolling sidedefs, a flat entry per view.  Through the seg walk (the fx pair: no
    fallback, and the frames differ from the same scene's with the effects off) and through the host walker, against the oracle's frame
    of the per-view WAD — the entries patched in, then the effects baked in at the view's timestamp (wall_fx.bake), since the oracle
    animates and scrolls no wall."""
    import wall_fx
    W, H = 131, 67
    wad = wall_fx.fx_wad()
    sides = sc.loaded_sides(wad)
    k = wall_fx.scroll_counts(wad)
    n = 24
    cases = []
    for v in range(n):
        e = [(i,) + tuple(t if t == "-" else "BFALL4" for t in sides[i][:3]) + (32760, 1) for i in range(len(sides)) if k[i]]
        for j, i in enumerate(range(v % 3, len(sides), 3)):
            if k[i]:
                continue
            tex = ("BFALL2", "SLADRIP3", "FIREWALB", "BRICK1", "BLODGR2")[(j + v) % 5]
            e.append((i,) + tuple(t if t == "-" else tex for t in sides[i][:3]) + (sides[i][3] + 5 + v, sides[i][4] - 3))
        e = e[:64]                                            # (the scrolling sidedefs come first and stay)
        cases.append(sc.Case(f"fx{v}", (41 * v + 40) % 1000, e, [(v % len(sc.loaded_flats(wad)), "NUKAGE2", "F_SKY1")], timestamp=float(np.float32(0.4 * v))))
    assert all(len(c.sides) <= 64 for c in cases)
    want = np.stack([sc.oracle_frame(oracle, wall_fx.bake(c.patched(wad), c.timestamp), c.record(path1993), W, H) for c in cases])
    views = dg.make_views(np.stack([c.record(path1993)[:8] for c in cases]))
    for i, c in enumerate(cases):
        views[i].timestamp = c.timestamp
    frames = {}
    for flags in (dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL, 0):
        s = dg.Scene(wad, "e1m1")
        nm = sc.Names(s)
        vf, keep = dg.make_view_surfaces([c.surfaces(nm) for c in cases])
        s.set_wall_effects(flags)
        for fe in (1, 3):
            ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
            ctx.upload_scene(s)
            before = ctx.fallbacks()
            frames[(flags, fe)] = ctx.render_surfaces(views, vf)
            if fe == 3:
                assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before and ctx.surface_timing(0) > 0.0
            ctx.close()
        s.close()
        del keep
    on = dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL
    _assert_frames(frames[(on, 3)], want, "wall effects, seg walk")
    _assert_frames(frames[(on, 1)], want, "wall effects, host walker")
    assert np.array_equal(frames[(0, 3)], frames[(0, 1)])
    assert sum(not np.array_equal(frames[(on, 3)][v], frames[(0, 3)][v]) for v in range(n)) >= n // 2      # the effects moved pixels: the fx variant ran


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_views_through_the_seg_walk_and_auto(dg, oracle, scene, names, wad, path1993, size):
    W, H = size
    n = 64
    cases = [c for c in sc.random_cases(wad, n, seed=4242)]
    for c in cases:                                           # (the side table holds 64 per frame on average: 64 of each view's third, spread over the whole index range)
        c.sides = [c.sides[(j * len(c.sides)) // 64] for j in range(64)] if len(c.sides) > 64 else c.sides
    assert max(e[0] for c in cases for e in c.sides) > len(sc.loaded_sides(wad)) * 0.9
    want = np.stack([sc.oracle_frame(oracle, c.patched(wad), c.record(path1993), W, H) for c in cases])
    vf, keep = dg.make_view_surfaces([c.surfaces(names) for c in cases])
    views = dg.make_views(np.stack([c.record(path1993)[:8] for c in cases]))
    for i, c in enumerate(cases):
        views[i].timestamp = c.timestamp
    for fe in (3, 0):
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        before = ctx.fallbacks()
        got = ctx.render_surfaces(views, vf)
        _assert_frames(got, want, ("dense", FE_NAMES[fe], size))
        print("dense:", FE_NAMES[fe], size, ctx.fallbacks(), ctx.timing(0)["front_end"])
        if fe == 3:                                           # the forced seg walk took the batch itself: no quiet fallback
            assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before and ctx.surface_timing(0) > 0.0
        assert np.array_equal(ctx.slot_sector_flats(0, 0, n), sc.expected_flat_rows(scene, names, cases))
        ctx.close()
    del keep


def test_bundle_with_surfaces(dg, scene, names, wad, path1993, pixel_batch):
    W, H = 131, 67
    n = 16
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vf, vs, poses, states, keep = _batch(dg, path1993, names, pixel_batch, n)
    assert {"grate_on", "grate_off"} <= {c.name for c in cases}
    ctx = dg.Context(W, H, max_batch=staging_cases.bundle_batch_for(dg, W, H, n), slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_bundle_surfaces(0, views, 7, vf, n=n, states=states, poses=poses, sectors=vs)
    _assert_frames(ctx.readback(0, 0, n), want, "bundle colour")
    dist, kind = ctx.readback_depth(0, 0, n)
    ids, cls, boxes = ctx.readback_labels(0, 0, n)
    grate_changed = 0
    for k in range(n):
        s2 = dg.Scene(cases[k].patched(wad), "e1m1")          # the product's own scene of the patched WAD: no entries needed
        lights, mobjs = pixel_batch["named_states"][k]
        for s, level in lights:
            s2.set_sector_light(s, level)
        for m, sp, fb in mobjs:
            s2.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
        fl, own = s2.build_lists_owners(W, H, views[k])
        frames = (dg.DgFrameLists * 1)(fl)
        d1, k1 = dg.depth_lists_host(s2, W, H, frames)
        i1, c1, b1 = dg.label_lists_host(s2, W, H, frames, [own])
        assert np.array_equal(dist[k], d1[0]) and np.array_equal(kind[k], k1[0]), k
        assert np.array_equal(ids[k], i1[0]) and np.array_equal(cls[k], c1[0]) and np.array_equal(boxes[k], b1[0]), k
        s2.close()
        if cases[k].name in ("grate_on", "grate_off"):        # the label plane's holes follow GRATE1: against the unchanged map's labels
            s3 = dg.Scene(wad, "e1m1")
            fl0, own0 = s3.build_lists_owners(W, H, views[k])
            i0, _, _ = dg.label_lists_host(s3, W, H, (dg.DgFrameLists * 1)(fl0), [own0])
            grate_changed += not np.array_equal(i0[0], ids[k])
            s3.close()
    assert grate_changed >= 1
    assert np.array_equal(ctx.slot_sector_flats(0, 0, n), sc.expected_flat_rows(scene, names, cases))
    assert ctx.surface_timing(0) == 0.0                       # (a bundle goes through the host lists)
    ctx.close()
    del keep


def test_redone_frames_keep_their_surfaces(dg, scene, names, path1993, pixel_batch, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=3 makes the device column walk overflow: frames are redone on the host at dg_wait, with their surfaces."""
    W, H = 320, 200
    n = 8
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vf, vs, poses, states, keep = _batch(dg, path1993, names, pixel_batch, n)
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "3")
    for fe in (2, 3):
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        ctx.submit_surfaces(0, views, vf, states=states, poses=poses, sectors=vs)
        ctx.wait(0)
        _assert_frames(ctx.readback(0, 0, n), want, ("redone", fe))
        counts = ctx.fallbacks()
        print("redone:", fe, counts)
        assert counts["front_end"] > 0 and counts["redone_frames"] > 0
        ctx.close()
    del keep


def test_redone_frames_read_only_the_slots_copy_of_the_inputs(dg, scene, names, path1993, pixel_batch, monkeypatch):
    """The same overflowing batch with all four inputs, and every entry array of the caller's overwritten with 0xFF bytes between the
    submission and dg_wait: the frames redone on the host at dg_wait are drawn from the slot's kept copy alone, so they are still the
    oracle's."""
    W, H = 320, 200
    n = 8
    want = pixel_batch["oracle"](W, H)[:n]
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "3")
    for fe in (2, 3):
        cases, views, vf, vs, poses, states, keep = _batch(dg, path1993, names, pixel_batch, n)
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        ctx.submit_surfaces(0, views, vf, states=states, poses=poses, sectors=vs)
        arrays = [a for k in keep for a in k]
        assert len(arrays) == 6 * n
        for a in arrays:
            ctypes.memset(a, 0xFF, ctypes.sizeof(a))
        ctx.wait(0)
        _assert_frames(ctx.readback(0, 0, n), want, ("redone from the kept copy", fe))
        counts = ctx.fallbacks()
        assert counts["front_end"] > 0 and counts["redone_frames"] > 0
        ctx.close()
        del keep


def test_replay_and_a_slot_reused_after_another_scene(dg, scene, names, wad1995, path1993, path1995, pixel_batch):
    W, H = 131, 67
    n = 16
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vf, vs, poses, states, keep = _batch(dg, path1993, names, pixel_batch, n)
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_surfaces(0, views, vf, states=states, poses=poses, sectors=vs)
    first = ctx.readback(0, 0, n)
    rows = ctx.slot_sector_flats(0, 0, n)
    ctx.submit(1, views)                                      # another slot's batch in between, without entries
    ctx.wait(1)
    ctx.replay(0)
    ctx.wait(0)
    _assert_frames(ctx.readback(0, 0, n), want, "replay")
    assert np.array_equal(first, ctx.readback(0, 0, n)) and np.array_equal(rows, ctx.slot_sector_flats(0, 0, n))
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS
    # another scene, with another sidedef and sector count
    other = dg.Scene(wad1995, "e1m1")
    assert other.sidedef_count() != scene.sidedef_count() and other.sector_count() != scene.sector_count()
    on = sc.Names(other)
    t, fsky, fl0 = on.texture("WIDE2"), on.flat_handle("F_SKY1"), on.flat_handle("FLOOR0")
    ctx.upload_scene(other)
    L = dg.lib()
    out = np.zeros((n, other.sector_count(), 2), dtype=np.int32)
    assert L.dg_slot_sector_flats(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE            # the upload emptied the slot
    three = dg.make_views(path1995[[100, 323, 640]])
    last_sd, last = other.sidedef_count() - 1, other.sector_count() - 1
    loaded = other.sidedef_surfaces()
    every = [(int(r[0]),) + tuple(int(x) if x < 0 else t for x in r[1:4]) + (3, 4) for r in loaded[::17]]
    one, keep2 = dg.make_view_surfaces([([(last_sd, t, t, t, 0, 0)] + every, [(last, fsky, fsky)]), ([], []), (every, [(0, fl0, fsky)])])
    got = ctx.render_surfaces(three, one)
    want_rows = np.repeat(other.sector_flats()[None, :, 1:], 3, axis=0)
    want_rows[0, last] = (fsky, fsky)
    want_rows[2, 0] = (fl0, fsky)
    assert np.array_equal(ctx.slot_sector_flats(0, 0, 3), want_rows) and ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS
    ref = dg.Context(W, H, max_batch=3, slots=1, front_end=dg_fe(dg, 1))
    ref.upload_scene(other)
    assert np.array_equal(got, ref.render_surfaces(three, one)) and not np.array_equal(got, ref.render(three))
    ref.close()
    ctx.close()
    other.close()
    del keep, keep2


def test_errors_of_the_slot_calls(dg, scene, names, path1993):
    W, H = 131, 67
    n_sd, n = scene.sidedef_count(), scene.sector_count()
    t, f = names.texture("BRICK1"), names.flat_handle("FLOOR0")
    ctx = dg.Context(W, H, max_batch=4, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    L = dg.lib()
    out = np.zeros((4, n, 2), dtype=np.int32)
    assert L.dg_slot_sector_flats(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE            # an empty slot
    views = dg.make_views(path1993[[100, 323, 640]])
    bad_sets = [([(n_sd, t, t, t, 0, 0)], []), ([(-1, t, t, t, 0, 0)], []), ([(0, -2, t, t, 0, 0)], []), ([(0, t, 1 << 24, t, 0, 0)], []), ([(0, t, t, t, 32768, 0)], []),
                ([(0, t, t, t, 0, -32769)], []), ([], [(n, f, f)]), ([], [(0, -1, f)]), ([], [(0, f, 1 << 28)])]
    for fe_ctx in (ctx,):
        for bad in bad_sets:
            vf, keep = dg.make_view_surfaces([([], []), bad, ([], [])])
            with pytest.raises(dg.DoomGpuError) as e:
                fe_ctx.submit_surfaces(0, views, vf)
            assert e.value.code == dg.DG_ERR_INVALID and "frame 1" in str(e.value), bad
    ctx.submit_map(1, views)
    assert L.dg_slot_sector_flats(ctx._h, 1, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE            # a 2-D map submission
    ctx.submit(0, views)
    assert L.dg_slot_sector_flats(ctx._h, 0, 0, 3, None) == dg.DG_ERR_INVALID
    assert L.dg_slot_sector_flats(ctx._h, 0, 2, 2, out.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_slot_sector_flats(ctx._h, 0, 0, 3, out.ctypes.data) == dg.DG_OK
    assert np.array_equal(out[:3], np.repeat(scene.sector_flats()[None, :, 1:], 3, axis=0))
    null_array = (dg.DgViewSurfaces * 3)(dg.DgViewSurfaces(None, 0, None, 0), dg.DgViewSurfaces(None, 2, None, 0), dg.DgViewSurfaces(None, 0, None, 0))
    assert L.dg_submit_views_surfaces(ctx._h, 0, views, None, None, None, null_array, 3) == dg.DG_ERR_INVALID and b"frame 1" in L.dg_last_error()
    assert L.dg_submit_bundle_views_surfaces(ctx._h, 0, views, None, None, None, null_array, 3, 1) == dg.DG_ERR_INVALID
    ctx.close()
    for fe in (1, 2):                                        # the host walker names the frame too
        c2 = dg.Context(W, H, max_batch=4, slots=1, front_end=dg_fe(dg, fe))
        c2.upload_scene(scene)
        for bad in (bad_sets[0], bad_sets[3], bad_sets[7]):
            vf, keep = dg.make_view_surfaces([([], []), ([], []), bad])
            with pytest.raises(dg.DoomGpuError) as e:
                c2.submit_surfaces(0, views, vf)
            assert e.value.code == dg.DG_ERR_INVALID and "frame 2" in str(e.value)
        c2.close()


def test_a_scene_that_loaded_flats_after_the_upload_is_refused(dg, wad, path1993):
    s = dg.Scene(wad, "e1m1")
    ctx = dg.Context(131, 67, max_batch=2, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(s)
    views = dg.make_views(path1993[[100, 323]])
    ctx.render(views)
    s.use_flat("EXTRAFL")
    with pytest.raises(dg.DoomGpuError) as e:
        ctx.render(views)
    assert e.value.code == dg.DG_ERR_INVALID and "upload it again" in str(e.value)
    ctx.upload_scene(s)
    ctx.render(views)
    ctx.close()
    s.close()


MIRROR_SRC = r'''
// Three ticks of Game::render through the mirror: the surfaces as loaded, then one sidedef's textures and one sector's flats changed and
// pushed through doom::sync_surfaces, then back; each Renderer draws with what the World then holds.
#include "doom-rust-renderer_amd/csrc/doomgpu.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
int main(int argc, char **argv) {
    if (argc < 14) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const doom::Player pl{{std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)}, std::strtof(argv[8], nullptr), std::strtof(argv[7], nullptr)};
    const int sidedef = std::atoi(argv[9]), sector = std::atoi(argv[11]);
    try {
        doom::World world(wad, "e1m1");
        const int tex = world.use_texture(argv[10]), floor_flat = world.use_flat(argv[12]), ceil_flat = world.use_flat(argv[13]);
        if (world.use_texture("-") != DG_TEX_NONE) return 5;
        doom::Device dev(W, H);
        dev.upload(world);
        std::FILE *out = std::fopen(argv[4], "wb");
        const std::vector<dg_side_surface> sides0 = world.sidedefs();
        const std::vector<dg_sector_flats> flats0 = world.sector_flats();
        if (sidedef < 0 || sidedef >= (int)sides0.size() || sector < 0 || sector >= (int)flats0.size()) return 3;
        for (int tick = 0; tick < 3; tick++) {
            std::vector<dg_side_surface> sides = sides0;
            std::vector<dg_sector_flats> flats = flats0;
            if (tick == 1) {
                dg_side_surface &s = sides[(size_t)sidedef];
                if (s.tex_mid >= 0) s.tex_mid = tex;
                if (s.tex_low >= 0) s.tex_low = tex;
                if (s.tex_up >= 0) s.tex_up = tex;
                s.x_offset += 9;
                flats[(size_t)sector].floor_flat = floor_flat;
                flats[(size_t)sector].ceil_flat = ceil_flat;
            }
            doom::sync_surfaces(world, sides, flats);
            if ((int)world.changed_sidedefs().size() != (tick == 1 ? 1 : 0) || (int)world.changed_flats().size() != (tick == 1 ? 1 : 0)) return 4;
            doom::Pixels pixels(W, H);
            doom::Renderer(pixels, world, pl, 0.0f, dev).render();
            std::fwrite(pixels.pixels.data(), 1, pixels.pixels.size(), out);
        }
        std::fclose(out);
    } catch (const doom::Error &e) { std::fprintf(stderr, "doom::Error %d: %s\n", e.code, e.what()); return 1; }
    return 0;
}
'''


def test_cpp_mirror_with_surfaces_changed_between_two_renders(tmp_path, dg, oracle, wad, path1993, campath_mod, pixel_batch):
    W, H = 320, 200
    c = next(c for c in pixel_batch["cases"] if c.name == "wide")
    sd, f = c.sides[0][0], c.frame
    loaded = sc.loaded_sides(wad)[sd]
    sector = next(s for fr, s in sc.visible_pairs(oracle, wad, path1993)[1] if fr == f)
    r = path1993[f]
    (tmp_path / "surfaces.cpp").write_text(MIRROR_SRC)
    (tmp_path / "synth.wad").write_bytes(wad)
    exe = tmp_path / "surfaces"
    lib = os.path.join(ROOT, "doom-rust-renderer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, str(tmp_path / "surfaces.cpp"), "-o", str(exe), os.path.join(lib, "libdoomgpu.so"), "-Wl,-rpath," + lib])
    run = subprocess.run([str(exe), str(tmp_path / "synth.wad"), str(W), str(H), str(tmp_path / "frames.rgb"), float(r[0]).hex(), float(r[1]).hex(), float(r[2]).hex(),
                          float(r[7]).hex(), str(sd), "EXTRA1", str(sector), "NUKAGE3", "F_SKY1"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    frames = np.fromfile(tmp_path / "frames.rgb", dtype=np.uint8).reshape(3, H, W, 3)
    rec = campath_mod.view_record(np.float32(r[0]), np.float32(r[1]), np.float32(r[2]), np.float32(r[7]))
    case = sc.Case("mirror", f, [(sd,) + tuple(n if n == "-" else "EXTRA1" for n in loaded[:3]) + (loaded[3] + 9, loaded[4])], [(sector, "NUKAGE3", "F_SKY1")])
    plain = sc.oracle_frame(oracle, wad, rec, W, H)
    moved = sc.oracle_frame(oracle, case.patched(wad), rec, W, H)
    assert np.array_equal(frames[0], plain) and np.array_equal(frames[1], moved) and np.array_equal(frames[2], plain)
    assert not np.array_equal(plain, moved)
