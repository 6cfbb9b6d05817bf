"""Per-view map-object poses on the GPU (include/doomgpu.h: dg_view_poses).  Everything is byte-exact.

  rows        the rows the pose kernels write for the seg walk (dg_slot_mobj_poses) equal the scene's rows with the entries applied and
              dg_scene_sectors_at's sectors: batches of 1, 3, 64 and 65 frames, entry totals at the kernels' boundaries, points on and next
              to partition lines, on vertices, NaN / infinite, and a map with holes; the seg walk keeps its path and its counters;
              on the hand world's oblique partition the points at which a fused side test finds the other sector, and exact ties
  pixels      72 views with a different pose set each, and light and state entries on top, through every front end against the oracle's
              frames of the per-view patched WADs; poses == NULL is dg_submit_views_state
  bundle      colour, depth and labels of posed views from one submission; a moved object's box moves with it
  redone      frames redone on the host after a column overflow keep their poses
  replay      dg_replay_slot of a pose batch reproduces it
  scene       a slot reused after dg_upload_scene of another scene sees that scene's rows
"""
import numpy as np
import pytest

import mobj_pose_cases as mp
import staging_cases
import walk_cases

pytestmark = pytest.mark.gpu

SIZES = [(320, 200), (131, 67)]
N_PIXELS = 72
FE_NAMES = {1: "host", 2: "device", 3: "device_segs", 0: "auto"}
F = np.float32


@pytest.fixture(scope="module")
def scene(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    for sprite, frame in STATE_SPRITES:
        sc.sprite_frame(sprite, frame)                        # (decoded before any upload)
    return sc


@pytest.fixture(scope="module")
def holes(dg, wad1993):
    wad = walk_cases.holes_wad(wad1993)
    return wad, dg.Scene(wad, "e1m1")


def _bits(rows):
    return np.ascontiguousarray(rows).view(np.uint8)


def _tame(x, y):
    """A point an object may be DRAWN at in the rows tests: finite and inside the map's box.  The others (NaN, infinities, 3e38, the far
    ring) are given to objects the same view's state sets to S_NULL: their rows are written and compared, their sprites are not asked
    for — what the reference itself makes of a sprite at infinity is not this test's subject."""
    return np.isfinite(x) & np.isfinite(y) & (x > -64) & (x < 4160) & (y > -64) & (y < 3136)


def _entry_sets(rng, n_frames, n_mobjs, px, py, total):
    """`total` entries that stand, unique per (frame, object), plus a losing earlier entry for every fifth of them:
    -> (per-view entry lists, {(frame, object): (x, y, angle)})."""
    cells = rng.permutation(n_frames * n_mobjs)[:total]
    stand, views = {}, [[] for _ in range(n_frames)]
    for j, c in enumerate(cells):
        f, m = int(c) // n_mobjs, int(c) % n_mobjs
        k = int(rng.integers(len(px)))
        e = (m, float(px[k]), float(py[k]), float(F(rng.uniform(-7.0, 7.0))))
        if j % 5 == 0:
            views[f].append((m, 123.0, float("nan"), 0.5))    # (loses to the entry below)
        views[f].append(e)
        stand[(f, m)] = e[1:]
    return views, stand


def _check_rows(dg, ctx, scene, path, n_frames, views, stand, what):
    n_mobjs = scene.mobj_count()
    base = scene.mobj_poses()
    want = np.tile(base, (n_frames, 1))
    null_states = [[] for _ in range(n_frames)]
    for (f, m), (x, y, a) in stand.items():
        sec = int(scene.sectors_at([x], [y])[0])
        want[f, m] = (x, y, a, sec)
        if not _tame(F(x), F(y)):
            null_states[f].append((m, -1, 0))
    poses, keep = dg.make_view_poses(views)
    states, keep2 = dg.make_view_states([([], ms) for ms in null_states])
    before = ctx.fallbacks()
    vs = dg.make_views(path[[(7 * i + 3) % 1000 for i in range(n_frames)]])
    ctx.submit_poses(0, vs, poses, states=states)
    got = ctx.slot_mobj_poses(0, 0, n_frames)
    assert got.shape == (n_frames, n_mobjs)
    bad = np.argwhere(np.any(_bits(got).reshape(n_frames, n_mobjs, 16) != _bits(want).reshape(n_frames, n_mobjs, 16), axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first (frame, object) {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
    untouched = np.ones((n_frames, n_mobjs), dtype=bool)
    for (f, m) in stand:
        untouched[f, m] = False
    assert np.array_equal(_bits(got[untouched]), _bits(np.tile(base, (n_frames, 1))[untouched]))
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS, what
    assert ctx.fallbacks() == before, what
    # a part of the range, and the kernels' time
    if n_frames > 2:
        part = ctx.slot_mobj_poses(0, 1, n_frames - 2)
        assert np.array_equal(_bits(part), _bits(got[1:n_frames - 1]))
    assert ctx.mobj_pose_timing(0) > 0.0
    del keep, keep2


@pytest.mark.parametrize("n_frames", [1, 3, 64, 65])
@pytest.mark.parametrize("which", ["map", "holes"])
def test_the_rows_the_pose_kernels_write(dg, scene, holes, wad1993, path1993, n_frames, which):
    W, H = (320, 200) if which == "map" else (131, 67)
    wad, sc = (wad1993, scene) if which == "map" else holes
    px, py = mp.lookup_points(wad, seed=n_frames)
    if which == "holes":
        ring = walk_cases.far_ring(180)
        px, py = np.concatenate([px, ring[:, 0]]), np.concatenate([py, ring[:, 1]])
    n_mobjs = sc.mobj_count()
    cells = n_frames * n_mobjs
    ctx = dg.Context(W, H, max_batch=65, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(sc)
    rng = np.random.default_rng(100 * n_frames + (which == "holes"))
    none_seen = 0
    for total in sorted({t for t in (0, 1, 63, 64, 65, 255, 256, 257, cells) if t <= cells}):
        views, stand = _entry_sets(rng, n_frames, n_mobjs, px, py, total)
        _check_rows(dg, ctx, sc, path1993, n_frames, views, stand, (which, n_frames, total))
        none_seen += sum(int(sc.sectors_at([x], [y])[0]) < 0 for (x, y, a) in stand.values())
    if which == "holes" and n_frames >= 3:
        assert none_seen > 0                                   # rows with sector -1 were among them
    ctx.close()


def test_entries_on_the_partition_line_of_the_hand_world(dg):
    """mobj_pose_cases.line_points as pose entries, four objects to a frame: points at which pose_sector_at's side test is 0.0 and a fused
    one is not (the import asserts sector 0 by the rule and 1 fused), and exact ties.  The rows' sectors equal the host's and the numpy
    descent's; a library built with contraction on fails here."""
    xs, ys, n = mp.line_points()
    sc = dg.Scene(mp.fc.wad_of("hand"), "e1m1")
    n_mobjs = sc.mobj_count()
    n_frames = -(-len(xs) // n_mobjs)
    entries = [[(i - f * n_mobjs, float(xs[i]), float(ys[i]), float(F(0.01 * i))) for i in range(f * n_mobjs, min(len(xs), (f + 1) * n_mobjs))] for f in range(n_frames)]
    poses, keep = dg.make_view_poses(entries)
    views = (dg.DgView * n_frames)(*[dg.DgView(96.0, 180.0, 0.0, 41.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1)] * n_frames)
    ctx = dg.Context(131, 67, max_batch=n_frames, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(sc)
    ctx.submit_poses(0, views, poses)
    rows = ctx.slot_mobj_poses(0, 0, n_frames)
    got = rows["sector"].reshape(-1)[:len(xs)]
    assert np.array_equal(rows["x"].reshape(-1)[:len(xs)].view(np.uint32), xs.view(np.uint32))
    host, model = sc.sectors_at(xs, ys), mp.line_sectors(xs, ys)
    print(f"pose rows whose sector differs from the host's: {int((got != host).sum())}, from the numpy descent's: {int((got != model).sum())} of {len(xs)}")
    assert np.array_equal(got, host) and np.array_equal(got, model)
    assert (got[:n] == 0).all() and set(got[n:].tolist()) == {0, 1}
    ctx.close()
    sc.close()
    del keep


def dg_fe(dg, fe):
    return {0: dg.DG_FE_AUTO, 1: dg.DG_FE_HOST, 2: dg.DG_FE_DEVICE, 3: dg.DG_FE_DEVICE_SEGS}[fe]


STATE_SPRITES = [("TROO", 0), ("BAR1", 0), ("CAND", 0)]


def _view_state(v, n_sectors, n_mobjs):
    """The game state of view v of the pixel batch: a light entry, a state entry, and every third view an S_NULL."""
    sprite, frame = STATE_SPRITES[v % len(STATE_SPRITES)]
    lights = [((v * 3) % n_sectors, 96 + (v * 16) % 160)]
    mobjs = [((v * 5 + 1) % n_mobjs, (sprite, frame), v % 2)] + ([((v * 5 + 2) % n_mobjs, None, 0)] if v % 3 == 0 else [])
    return lights, mobjs


@pytest.fixture(scope="module")
def pixel_batch(dg, oracle, scene, wad1993, path1993):
    """The 72 cases, their poses and states as the product takes them, and per size the oracle's frames."""
    cases = mp.batch_cases(scene, wad1993, path1993, N_PIXELS)
    n_sectors, n_mobjs = scene.sector_count(), scene.mobj_count()
    st = [_view_state(v, n_sectors, n_mobjs) for v in range(N_PIXELS)]

    def prepare(osc, k):
        lights, mobjs = st[k]
        for s, level in lights:
            osc.set_sector_light(s, level)
        for m, sp, fb in mobjs:
            osc.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
    frames = {}

    def oracle_for(W, H):
        if (W, H) not in frames:
            frames[(W, H)] = mp.oracle_frames(oracle, wad1993, path1993, cases, W, H, prepare=prepare)
        return frames[(W, H)]
    states = [(lights, [(m, scene.sprite_frame(*sp) if sp else -1, fb) for m, sp, fb in mobjs]) for lights, mobjs in st]
    return {"cases": cases, "entries": [mp.entries_as_poses(c.entries) for c in cases], "states": states, "named_states": st, "oracle": oracle_for}


def _batch(dg, path, pixel_batch, n):
    """The first n views of the pixel batch as the calls take them: (cases, views, poses, states, keep-alive)."""
    cases = pixel_batch["cases"][:n]
    poses, keep = dg.make_view_poses(pixel_batch["entries"][:n])
    states, keep2 = dg.make_view_states(pixel_batch["states"][:n])
    return cases, dg.make_views(path[[c.frame for c in cases]]), poses, states, (keep, keep2)


def _assert_frames(got, want, what):
    for k in range(len(want)):
        bad = np.argwhere(np.any(got[k] != want[k], axis=2))
        assert len(bad) == 0, f"{what}: view {k}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fe", [1, 2, 3, 0], ids=lambda f: FE_NAMES[f])
def test_pixels_equal_the_oracle_of_the_patched_wads(dg, scene, wad1993, path1993, pixel_batch, fe, size):
    W, H = size
    want = pixel_batch["oracle"](W, H)
    mp.assert_formula(scene, wad1993)
    cases, views, poses, states, keep = _batch(dg, path1993, pixel_batch, N_PIXELS)
    ctx = dg.Context(W, H, max_batch=N_PIXELS, slots=1, front_end=dg_fe(dg, fe))
    ctx.upload_scene(scene)
    before = ctx.fallbacks()
    got = ctx.render_poses(views, poses, states=states)
    _assert_frames(got, want, (FE_NAMES[fe], size))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before
    # the rows every front end says it drew with: the entries applied to the scene's rows
    rows = ctx.slot_mobj_poses(0, 0, N_PIXELS)
    base = scene.mobj_poses()
    for k, c in enumerate(cases):
        row = base.copy()
        for m, x, y, a in mp.entries_as_poses([(m,) + v for m, v in mp.resolved(c.entries).items()]):
            row[m] = (x, y, a, int(scene.sectors_at([x], [y])[0]))
        assert np.array_equal(_bits(rows[k]), _bits(row)), (FE_NAMES[fe], k)
    # poses == NULL is dg_submit_views_state, byte for byte
    plain = ctx.render_state(views, states)
    ctx.submit_poses(0, views, None, states=states)
    assert np.array_equal(ctx.readback(0, 0, N_PIXELS), plain)
    assert np.array_equal(_bits(ctx.slot_mobj_poses(0, 0, 2)), _bits(np.tile(base, (2, 1))))
    assert ctx.mobj_pose_timing(0) == 0.0
    assert not np.array_equal(plain, got)
    ctx.close()
    del keep


def test_errors_of_the_slot_calls(dg, scene, path1993):
    W, H = 131, 67
    n = scene.mobj_count()
    ctx = dg.Context(W, H, max_batch=4, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    L = dg.lib()
    out = np.zeros((4, n), dtype=dg.MOBJ_PLACED_DTYPE)
    assert L.dg_slot_mobj_poses(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # an empty slot
    views = dg.make_views(path1993[[100, 323, 640]])
    for bad in (n, -1):
        poses, keep = dg.make_view_poses([[], [(0, 1.0, 2.0, 3.0), (bad, 1.0, 2.0, 3.0)], []])
        with pytest.raises(dg.DoomGpuError) as e:
            ctx.submit_poses(0, views, poses)
        assert e.value.code == dg.DG_ERR_INVALID and "frame 1" in str(e.value)
    ctx.submit_map(1, views)
    assert L.dg_slot_mobj_poses(ctx._h, 1, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # a 2-D map submission
    ctx.submit(0, views)
    assert L.dg_slot_mobj_poses(ctx._h, 0, 0, 3, None) == dg.DG_ERR_INVALID
    assert L.dg_slot_mobj_poses(ctx._h, 0, 2, 2, out.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_slot_mobj_poses(ctx._h, 0, 0, 3, out.ctypes.data) == dg.DG_OK
    null_array = (dg.DgViewPoses * 3)(dg.DgViewPoses(None, 0), dg.DgViewPoses(None, 2), dg.DgViewPoses(None, 0))
    assert L.dg_submit_views_poses(ctx._h, 0, views, None, null_array, 3) == dg.DG_ERR_INVALID
    assert L.dg_submit_bundle_views_poses(ctx._h, 0, views, None, null_array, 3, 1) == dg.DG_ERR_INVALID
    ctx.close()
    for fe in (1, 2):                                        # the host walker names the frame too
        c2 = dg.Context(W, H, max_batch=4, slots=1, front_end=dg_fe(dg, fe))
        c2.upload_scene(scene)
        poses, keep = dg.make_view_poses([[], [], [(n + 3, 1.0, 2.0, 3.0)]])
        with pytest.raises(dg.DoomGpuError) as e:
            c2.submit_poses(0, views, poses)
        assert e.value.code == dg.DG_ERR_INVALID and "frame 2" in str(e.value)
        c2.close()


def test_bundle_with_poses(dg, scene, wad1993, path1993, pixel_batch):
    W, H = 131, 67
    n = 12
    want = pixel_batch["oracle"](W, H)[:n]
    entries = pixel_batch["entries"]
    cases, views, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    ctx = dg.Context(W, H, max_batch=staging_cases.bundle_batch_for(dg, W, H, n), slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_bundle_poses(0, views, 7, poses, n=n, states=states)
    _assert_frames(ctx.readback(0, 0, n), want, "bundle colour")
    dist, kind = ctx.readback_depth(0, 0, n)
    ids, cls, boxes = ctx.readback_labels(0, 0, n)
    # the same parts from the lists of dg_build_lists_poses.  The list builder takes no view state: each view's light and state entries
    # are set on a scene of its own.
    moved_boxes = 0
    for k in range(n):
        sc = dg.Scene(wad1993, "e1m1")
        lights, mobjs = pixel_batch["named_states"][k]
        for s, level in lights:
            sc.set_sector_light(s, level)
        for m, sp, fb in mobjs:
            sc.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
        fl, own = sc.build_lists_poses(W, H, views[k], entries[k], owners=True)
        frames = (dg.DgFrameLists * 1)(fl)
        d1, k1 = dg.depth_lists_host(sc, W, H, frames)
        i1, c1, b1 = dg.label_lists_host(sc, W, H, frames, [own])
        assert np.array_equal(dist[k], d1[0]) and np.array_equal(kind[k], k1[0]), k
        assert np.array_equal(ids[k], i1[0]) and np.array_equal(cls[k], c1[0]) and np.array_equal(boxes[k], b1[0]), k
        # a moved object's box moves with it: against the labels of the same view without poses
        fl0, own0 = sc.build_lists_owners(W, H, views[k])
        _, _, b0 = dg.label_lists_host(sc, W, H, (dg.DgFrameLists * 1)(fl0), [own0], id=False, cls=False)
        for m in mp.resolved(cases[k].entries):
            px = int(((ids[k] == m) & (cls[k] == dg.DG_LABEL_MOBJ)).sum())
            assert int(boxes[k][m]["pixels"]) == px
            moved_boxes += px > 0 and boxes[k][m] != b0[0][m]
        sc.close()
    assert moved_boxes >= 3
    rows = ctx.slot_mobj_poses(0, 0, n)
    assert int(rows[0]["sector"][0]) >= -1 and rows.shape == (n, scene.mobj_count())
    ctx.close()
    del keep


def test_redone_frames_keep_their_poses(dg, scene, path1993, pixel_batch, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=3 makes the device column walk overflow: frames are redone on the host at dg_wait, with their poses."""
    W, H = 320, 200
    n = 8
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "3")
    for fe in (2, 3):
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        ctx.submit_poses(0, views, poses, states=states)
        ctx.wait(0)
        _assert_frames(ctx.readback(0, 0, n), want, ("redone", fe))
        counts = ctx.fallbacks()
        print("redone:", fe, counts)
        assert counts["front_end"] > 0 and counts["redone_frames"] > 0
        ctx.close()
    del keep


def test_replay_reproduces_a_pose_batch(dg, scene, path1993, pixel_batch):
    W, H = 131, 67
    n = 16
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_poses(0, views, poses, states=states)
    first = ctx.readback(0, 0, n)
    rows = ctx.slot_mobj_poses(0, 0, n)
    ctx.submit(1, views)                                      # another slot's batch in between, without poses
    ctx.wait(1)
    ctx.replay(0)
    ctx.wait(0)
    _assert_frames(ctx.readback(0, 0, n), want, "replay")
    assert np.array_equal(first, ctx.readback(0, 0, n))
    assert np.array_equal(_bits(rows), _bits(ctx.slot_mobj_poses(0, 0, n)))
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS
    ctx.close()
    del keep


def test_a_slot_reused_after_another_scene_sees_no_stale_rows(dg, scene, holes, path1993):
    W, H = 131, 67
    n = 3
    _, other = holes
    views = dg.make_views(path1993[[100, 323, 640]])
    moved = [[(m, float(path1993[(100 + 4 * m) % 1000][0]), float(path1993[(100 + 4 * m) % 1000][1]), 1.0) for m in range(scene.mobj_count())]] * n
    poses, keep = dg.make_view_poses(moved)
    ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    with_poses = ctx.render_poses(views, poses)
    ctx.upload_scene(other)
    L = dg.lib()
    out = np.zeros((n, other.mobj_count()), dtype=dg.MOBJ_PLACED_DTYPE)
    assert L.dg_slot_mobj_poses(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # the upload emptied the slot
    one, keep2 = dg.make_view_poses([[(0, 1000.0, 1000.0, 0.0)], [], []])
    got = ctx.render_poses(views, one)
    rows = ctx.slot_mobj_poses(0, 0, n)
    base = other.mobj_poses()
    want = np.tile(base, (n, 1))
    want[0, 0] = (1000.0, 1000.0, 0.0, int(other.sectors_at([1000.0], [1000.0])[0]))
    assert np.array_equal(_bits(rows), _bits(want))
    ref = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, 1))
    ref.upload_scene(other)
    assert np.array_equal(got, ref.render_poses(views, one))
    assert not np.array_equal(got, with_poses)
    ref.close()
    ctx.close()
    del keep, keep2
