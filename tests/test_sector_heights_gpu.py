"""Per-view sector heights on the GPU (include/doomgpu.h: dg_view_sectors).  Everything is byte-exact.

  rows        the rows the row kernels write for the seg walk (dg_slot_sector_heights) equal the scene's heights with the entries
              applied: batches of 1, 3, 64 and 65 frames, entry totals at the kernels' boundaries and every cell, a losing earlier entry
              for every fifth, the int16 limits among the heights; the seg walk keeps its path and its counters
  pixels      72 views with a different set of moved sectors each, and light, state and pose entries on top, through every front end
              against the oracle's frames of the per-view patched WADs; with the wall effects on through the fx pair
  wild        64 views with every sector at random heights, through the seg walk and DG_FE_AUTO, whichever frames are handed back
  bundle      colour, depth and labels from one submission; in `rides` the object's box moves down with the floor
  redone      frames redone on the host after a column overflow keep their heights
  replay      dg_replay_slot of a batch with entries reproduces it; a slot reused after another scene sees that scene's heights
  mirror      doomgpu.hpp with a sector lowered between two render() calls
"""
import os
import subprocess

import numpy as np
import pytest

import mobj_pose_cases as mp
import sector_height_cases as sh
import staging_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [(320, 200), (131, 67)]
N_PIXELS = 72
FE_NAMES = {1: "host", 2: "device", 3: "device_segs", 0: "auto"}
STATE_SPRITES = [("TROO", 0), ("BAR1", 0), ("CAND", 0)]


def dg_fe(dg, fe):
    return {0: dg.DG_FE_AUTO, 1: dg.DG_FE_HOST, 2: dg.DG_FE_DEVICE, 3: dg.DG_FE_DEVICE_SEGS}[fe]


@pytest.fixture(scope="module")
def scene(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    for sprite, frame in STATE_SPRITES:
        sc.sprite_frame(sprite, frame)                        # (decoded before any upload)
    return sc


def _limit(rng):
    k = int(rng.integers(0, 12))
    return -32768 if k == 0 else 32767 if k == 1 else int(rng.integers(-600, 601))


def _entry_sets(rng, n_frames, n_sectors, total):
    """`total` entries that stand, unique per (frame, sector), plus a losing earlier entry for every fifth of them."""
    cells = rng.permutation(n_frames * n_sectors)[:total]
    views = [[] for _ in range(n_frames)]
    for j, c in enumerate(cells):
        f, s = int(c) // n_sectors, int(c) % n_sectors
        if j % 5 == 0:
            views[f].append((s, 12345, -12345))               # (loses to the entry below)
        views[f].append((s, _limit(rng), _limit(rng)))
    return views


@pytest.mark.parametrize("n_frames", [1, 3, 64, 65])
def test_the_rows_the_row_kernels_write(dg, scene, wad1993, path1993, n_frames):
    W, H = SIZES[n_frames % 2]
    n_sectors = scene.sector_count()
    cells = n_frames * n_sectors
    base = sh.loaded_heights(wad1993)
    ctx = dg.Context(W, H, max_batch=65, slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    rng = np.random.default_rng(100 * n_frames)
    views = dg.make_views(path1993[[(7 * i + 3) % 1000 for i in range(n_frames)]])
    limits_seen = 0
    for total in sorted({t for t in (0, 1, 63, 64, 65, 255, 256, 257, cells) if t <= cells}):
        sets = _entry_sets(rng, n_frames, n_sectors, total)
        want = sh.expected_rows(wad1993, [sh.Case("", 0, e) for e in sets])
        limits_seen += int(((want == -32768) | (want == 32767)).sum())
        vs, keep = dg.make_view_sectors(sets)
        before = ctx.fallbacks()
        ctx.submit_sectors(0, views, vs)
        got = ctx.slot_sector_heights(0, 0, n_frames)
        assert got.shape == (n_frames, n_sectors, 2) and got.dtype == np.int16
        bad = np.argwhere(np.any(got != want, axis=2))
        assert len(bad) == 0, f"{(n_frames, total)}: {len(bad)} cells differ, first (frame, sector) {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
        assert (got != np.repeat(base[None], n_frames, axis=0)).any(axis=2).sum() <= total
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before, (n_frames, total)
        if n_frames > 2:                                      # a part of the range
            assert np.array_equal(ctx.slot_sector_heights(0, 1, n_frames - 2), got[1:n_frames - 1])
        assert ctx.sector_height_timing(0) > 0.0              # (an empty entry list still has its rows filled: sectors != NULL)
        ctx.submit_sectors(0, views, None)                    # no entries: neither kernel, the plain pair, the loaded heights
        assert ctx.sector_height_timing(0) == 0.0
        assert np.array_equal(ctx.slot_sector_heights(0, 0, n_frames), np.repeat(base[None], n_frames, axis=0))
        del keep
    assert limits_seen > 0
    ctx.close()


def _view_state(v, n_sectors, n_mobjs):
    sprite, frame = STATE_SPRITES[v % len(STATE_SPRITES)]
    lights = [((v * 3) % n_sectors, 96 + (v * 16) % 160)]
    mobjs = [((v * 5 + 1) % n_mobjs, (sprite, frame), v % 2)] + ([((v * 5 + 2) % n_mobjs, None, 0)] if v % 3 == 0 else [])
    return lights, mobjs


@pytest.fixture(scope="module")
def pixel_batch(dg, oracle, scene, wad1993, path1993):
    """The 72 cases — the named ones first, then one to five visible sectors moved per view — with light, state and pose entries on
    top, as the product takes them, and per size the oracle's frames of the per-view patched WADs."""
    pairs = sh.visible_pairs(oracle, wad1993, path1993)
    cases = sh.named_cases(scene, oracle, wad1993, path1993, pairs, sh.find_sky_pair(oracle, wad1993, path1993, pairs))
    hs = sh.loaded_heights(wad1993).astype(int)
    n_sectors, n_mobjs = scene.sector_count(), scene.mobj_count()
    by_frame = {}
    for f, s in pairs:
        by_frame.setdefault(f, []).append(s)
    frames = sorted(by_frame)
    moves = (lambda fl, ce: (fl, fl), lambda fl, ce: (fl + 16, ce), lambda fl, ce: (fl - 32, ce), lambda fl, ce: (fl, ce - 24))
    for v in range(len(cases), N_PIXELS):
        f = frames[(v * 3) % len(frames)]
        seen = by_frame[f]
        picked = []
        for j in range(v % 5 + 1):
            s = seen[(v + j) % len(seen)] if j < len(seen) else (v * 7 + j * 11) % n_sectors
            if s not in picked:
                picked.append(s)
        entries = [(s,) + tuple(moves[(v + j) % 4](hs[s, 0], hs[s, 1])) for j, s in enumerate(picked)]
        a = mp.ahead(path1993, f, 0)
        poses = [((v * 7) % n_mobjs,) + mp.target(path1993, f + a[v % len(a)]) + ((v * 29) % 360 - 180,)] if v % 2 == 0 and a else []
        cases.append(sh.Case(f"view{v}", f, entries, poses=poses))
    assert len({(c.frame, tuple(c.entries)) for c in cases}) == N_PIXELS          # a different set per view
    st = [_view_state(v, n_sectors, n_mobjs) for v in range(N_PIXELS)]
    frames_of = {}

    def oracle_for(W, H, cases_=cases, key="pixels"):
        if (W, H, key) not in frames_of:
            out = np.empty((len(cases_), H, W, 3), dtype=np.uint8)
            for k, c in enumerate(cases_):
                def prepare(osc, k=k):
                    lights, mobjs = st[k]
                    for s, level in lights:
                        osc.set_sector_light(s, level)
                    for m, sp, fb in mobjs:
                        osc.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
                out[k] = sh.oracle_frame(oracle, c.patched(wad1993), c.record(path1993), W, H, prepare=prepare)
            frames_of[(W, H, key)] = out
        return frames_of[(W, H, key)]
    states = [(lights, [(m, scene.sprite_frame(*sp) if sp else -1, fb) for m, sp, fb in mobjs]) for lights, mobjs in st]
    return {"cases": cases, "states": states, "named_states": st, "oracle": oracle_for}


def _batch(dg, path, pixel_batch, n):
    """The first n views of the pixel batch as the calls take them: (cases, views, sectors, poses, states, keep-alive)."""
    cases = pixel_batch["cases"][:n]
    vs, keep = dg.make_view_sectors([c.entries for c in cases])
    poses, keep2 = dg.make_view_poses([mp.entries_as_poses(c.poses) for c in cases])
    states, keep3 = dg.make_view_states(pixel_batch["states"][:n])
    return cases, dg.make_views(np.stack([c.record(path) for c in cases])), vs, poses, states, (keep, keep2, keep3)


def _assert_frames(got, want, what):
    for k in range(len(want)):
        bad = np.argwhere(np.any(got[k] != want[k], axis=2))
        assert len(bad) == 0, f"{what}: view {k}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fe", [1, 2, 3, 0], ids=lambda f: FE_NAMES[f])
def test_pixels_equal_the_oracle_of_the_patched_wads(dg, scene, wad1993, path1993, pixel_batch, fe, size):
    W, H = size
    want = pixel_batch["oracle"](W, H)
    cases, views, vs, poses, states, keep = _batch(dg, path1993, pixel_batch, N_PIXELS)
    ctx = dg.Context(W, H, max_batch=N_PIXELS, slots=1, front_end=dg_fe(dg, fe))
    ctx.upload_scene(scene)
    before = ctx.fallbacks()
    got = ctx.render_sectors(views, vs, states=states, poses=poses)
    _assert_frames(got, want, (FE_NAMES[fe], size))
    if fe == 3:
        assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before
        assert ctx.sector_height_timing(0) > 0.0 and ctx.mobj_pose_timing(0) > 0.0
    # the heights every front end says it drew with
    assert np.array_equal(ctx.slot_sector_heights(0, 0, N_PIXELS), sh.expected_rows(wad1993, cases)), FE_NAMES[fe]
    # sectors == NULL is dg_submit_views_poses, byte for byte
    plain = ctx.render_poses(views, poses, states=states)
    ctx.submit_sectors(0, views, None, states=states, poses=poses)
    assert np.array_equal(ctx.readback(0, 0, N_PIXELS), plain)
    assert ctx.sector_height_timing(0) == 0.0
    assert not np.array_equal(plain, got)
    ctx.close()
    del keep


def test_pixels_with_the_wall_effects_on_go_through_the_fx_pair(dg, wad1993, path1993, pixel_batch):
    """The scene's wall effects on: the seg walk of a batch with entries is the row-reading fx pair.  Reference: the host walker of the
    same scene (equal to the product's scene of the patched WAD with the same effects on the CPU tier)."""
    W, H = 131, 67
    sc = dg.Scene(wad1993, "e1m1")
    for sprite, frame in STATE_SPRITES:
        sc.sprite_frame(sprite, frame)
    sc.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
    cases, views, vs, poses, states, keep = _batch(dg, path1993, pixel_batch, N_PIXELS)
    for i in range(N_PIXELS):
        views[i].timestamp = 0.4 * i
    frames = {}
    for fe in (1, 3):
        ctx = dg.Context(W, H, max_batch=N_PIXELS, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(sc)
        before = ctx.fallbacks()
        frames[fe] = ctx.render_sectors(views, vs, states=states, poses=poses)
        if fe == 3:
            assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS and ctx.fallbacks() == before and ctx.sector_height_timing(0) > 0.0
            plain = ctx.render_poses(views, poses, states=states)
        ctx.close()
    _assert_frames(frames[3], frames[1], "wall effects")
    assert not np.array_equal(frames[3], plain)
    # one view against the oracle's pixels through the product's own scene of the patched WAD, with the effects on
    for k in (0, 20):
        patched = dg.Scene(cases[k].patched(wad1993), "e1m1")
        for sprite, frame in STATE_SPRITES:
            patched.sprite_frame(sprite, frame)
        patched.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
        ref = dg.Context(W, H, max_batch=1, slots=1, front_end=dg_fe(dg, 1))
        ref.upload_scene(patched)
        one_state, keep2 = dg.make_view_states(pixel_batch["states"][k:k + 1])
        one_view = dg.make_views(cases[k].record(path1993)[None], timestamp=0.4 * k)
        assert np.array_equal(ref.render_state(one_view, one_state)[0], frames[3][k]), k
        ref.close()
        patched.close()
    sc.close()
    del keep


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wild_rows_through_the_seg_walk_and_auto(dg, oracle, scene, wad1993, path1993, size):
    W, H = size
    n = 64
    cases = sh.random_cases(wad1993, n, seed=4242)
    want = np.stack([sh.oracle_frame(oracle, c.patched(wad1993), c.record(path1993), W, H) for c in cases])
    vs, keep = dg.make_view_sectors([c.entries for c in cases])
    views = dg.make_views(np.stack([c.record(path1993) for c in cases]))
    for fe in (3, 0):
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        got = ctx.render_sectors(views, vs)
        _assert_frames(got, want, ("wild", FE_NAMES[fe], size))
        print("wild:", FE_NAMES[fe], size, ctx.fallbacks(), ctx.timing(0)["front_end"])
        assert np.array_equal(ctx.slot_sector_heights(0, 0, n), sh.expected_rows(wad1993, cases))
        ctx.close()
    del keep


def test_bundle_with_sector_heights(dg, scene, wad1993, path1993, pixel_batch):
    W, H = 131, 67
    n = 16
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vs, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    assert "rides" in [c.name for c in cases]
    ctx = dg.Context(W, H, max_batch=staging_cases.bundle_batch_for(dg, W, H, n), slots=1, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_bundle_sectors(0, views, 7, vs, n=n, states=states, poses=poses)
    _assert_frames(ctx.readback(0, 0, n), want, "bundle colour")
    dist, kind = ctx.readback_depth(0, 0, n)
    ids, cls, boxes = ctx.readback_labels(0, 0, n)
    rode = False
    for k in range(n):
        sc = dg.Scene(wad1993, "e1m1")
        lights, mobjs = pixel_batch["named_states"][k]
        for s, level in lights:
            sc.set_sector_light(s, level)
        for m, sp, fb in mobjs:
            sc.set_mobj_state(m, sp[0] if sp else None, sp[1] if sp else 0, bool(fb))
        p = mp.entries_as_poses(cases[k].poses) if cases[k].poses else None
        fl, own = sc.build_lists_sectors(W, H, views[k], cases[k].entries, p, owners=True)
        frames = (dg.DgFrameLists * 1)(fl)
        d1, k1 = dg.depth_lists_host(sc, W, H, frames)
        i1, c1, b1 = dg.label_lists_host(sc, W, H, frames, [own])
        assert np.array_equal(dist[k], d1[0]) and np.array_equal(kind[k], k1[0]), k
        assert np.array_equal(ids[k], i1[0]) and np.array_equal(cls[k], c1[0]) and np.array_equal(boxes[k], b1[0]), k
        if cases[k].name == "rides":                          # the object's box moves down with the floor: against the same pose, floor unmoved
            m = cases[k].poses[0][0]
            fl0, own0 = sc.build_lists_poses(W, H, views[k], p, owners=True)
            _, _, b0 = dg.label_lists_host(sc, W, H, (dg.DgFrameLists * 1)(fl0), [own0], id=False, cls=False)
            assert int(boxes[k][m]["pixels"]) > 0 and int(b0[0][m]["pixels"]) > 0
            new, old = (int(boxes[k][m]["y0"]), int(boxes[k][m]["y1"])), (int(b0[0][m]["y0"]), int(b0[0][m]["y1"]))
            assert new[0] >= old[0] and new[1] >= old[1] and new != old, (boxes[k][m], b0[0][m])     # (an edge at the frame's bottom row stays there)
            rode = True
        sc.close()
    assert rode
    assert np.array_equal(ctx.slot_sector_heights(0, 0, n), sh.expected_rows(wad1993, cases))
    assert ctx.sector_height_timing(0) == 0.0                 # (a bundle goes through the host lists)
    ctx.close()
    del keep


def test_redone_frames_keep_their_heights(dg, scene, path1993, pixel_batch, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=3 makes the device column walk overflow: frames are redone on the host at dg_wait, with their heights."""
    W, H = 320, 200
    n = 8
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vs, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "3")
    for fe in (2, 3):
        ctx = dg.Context(W, H, max_batch=n, slots=1, front_end=dg_fe(dg, fe))
        ctx.upload_scene(scene)
        ctx.submit_sectors(0, views, vs, states=states, poses=poses)
        ctx.wait(0)
        _assert_frames(ctx.readback(0, 0, n), want, ("redone", fe))
        counts = ctx.fallbacks()
        print("redone:", fe, counts)
        assert counts["front_end"] > 0 and counts["redone_frames"] > 0
        ctx.close()
    del keep


def test_replay_and_a_slot_reused_after_another_scene(dg, scene, wad1993, wad1995, path1993, path1995, pixel_batch):
    W, H = 131, 67
    n = 16
    want = pixel_batch["oracle"](W, H)[:n]
    cases, views, vs, poses, states, keep = _batch(dg, path1993, pixel_batch, n)
    ctx = dg.Context(W, H, max_batch=n, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    ctx.submit_sectors(0, views, vs, states=states, poses=poses)
    first = ctx.readback(0, 0, n)
    rows = ctx.slot_sector_heights(0, 0, n)
    ctx.submit(1, views)                                      # another slot's batch in between, without entries
    ctx.wait(1)
    ctx.replay(0)
    ctx.wait(0)
    _assert_frames(ctx.readback(0, 0, n), want, "replay")
    assert np.array_equal(first, ctx.readback(0, 0, n)) and np.array_equal(rows, ctx.slot_sector_heights(0, 0, n))
    assert ctx.timing(0)["front_end"] == dg.DG_FE_DEVICE_SEGS
    # another scene, with another sector count
    other_wad = wad1995                                       # (108 sectors against 105)
    other = dg.Scene(other_wad, "e1m1")
    assert other.sector_count() != scene.sector_count()
    ctx.upload_scene(other)
    L = dg.lib()
    out = np.zeros((n, other.sector_count(), 2), dtype=np.int16)
    assert L.dg_slot_sector_heights(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # the upload emptied the slot
    three = dg.make_views(path1995[[100, 323, 640]])
    last = other.sector_count() - 1
    one, keep2 = dg.make_view_sectors([[(last, -40, 8)], [], [(0, 3, 3)]])
    got = ctx.render_sectors(three, one)
    want_rows = sh.expected_rows(other_wad, [sh.Case("", 0, [(last, -40, 8)]), sh.Case("", 0, []), sh.Case("", 0, [(0, 3, 3)])])
    assert np.array_equal(ctx.slot_sector_heights(0, 0, 3), want_rows)
    ref = dg.Context(W, H, max_batch=3, slots=1, front_end=dg_fe(dg, 1))
    ref.upload_scene(other)
    assert np.array_equal(got, ref.render_sectors(three, one))
    ref.close()
    ctx.close()
    other.close()
    del keep, keep2


def test_errors_of_the_slot_calls(dg, scene, path1993):
    W, H = 131, 67
    n = scene.sector_count()
    ctx = dg.Context(W, H, max_batch=4, slots=2, front_end=dg_fe(dg, 3))
    ctx.upload_scene(scene)
    L = dg.lib()
    out = np.zeros((4, n, 2), dtype=np.int16)
    assert L.dg_slot_sector_heights(ctx._h, 0, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # an empty slot
    views = dg.make_views(path1993[[100, 323, 640]])
    for bad in ((n, 0, 0), (-1, 0, 0), (0, 32768, 0), (0, 0, -32769)):
        vs, keep = dg.make_view_sectors([[], [(0, 1, 2), bad], []])
        with pytest.raises(dg.DoomGpuError) as e:
            ctx.submit_sectors(0, views, vs)
        assert e.value.code == dg.DG_ERR_INVALID and "frame 1" in str(e.value)
    ctx.submit_map(1, views)
    assert L.dg_slot_sector_heights(ctx._h, 1, 0, 1, out.ctypes.data) == dg.DG_ERR_STATE          # a 2-D map submission
    ctx.submit(0, views)
    assert L.dg_slot_sector_heights(ctx._h, 0, 0, 3, None) == dg.DG_ERR_INVALID
    assert L.dg_slot_sector_heights(ctx._h, 0, 2, 2, out.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_slot_sector_heights(ctx._h, 0, 0, 3, out.ctypes.data) == dg.DG_OK
    null_array = (dg.DgViewSectors * 3)(dg.DgViewSectors(None, 0), dg.DgViewSectors(None, 2), dg.DgViewSectors(None, 0))
    assert L.dg_submit_views_sectors(ctx._h, 0, views, None, None, null_array, 3) == dg.DG_ERR_INVALID
    assert L.dg_submit_bundle_views_sectors(ctx._h, 0, views, None, None, null_array, 3, 1) == dg.DG_ERR_INVALID
    ctx.close()
    for fe in (1, 2):                                        # the host walker names the frame too
        c2 = dg.Context(W, H, max_batch=4, slots=1, front_end=dg_fe(dg, fe))
        c2.upload_scene(scene)
        vs, keep = dg.make_view_sectors([[], [], [(n + 3, 1, 2)]])
        with pytest.raises(dg.DoomGpuError) as e:
            c2.submit_sectors(0, views, vs)
        assert e.value.code == dg.DG_ERR_INVALID and "frame 2" in str(e.value)
        c2.close()


MIRROR_SRC = r'''
// Two ticks of Game::render through the mirror: the sectors as loaded, then one of them moved (a door, a lift) and pushed through
// doom::sync_state; the second Renderer draws with it.
#include "doom-rust-renderer_amd/csrc/doomgpu.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
int main(int argc, char **argv) {
    if (argc < 12) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const doom::Player pl{{std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)}, std::strtof(argv[8], nullptr), std::strtof(argv[7], nullptr)};
    const int sector = std::atoi(argv[9]);
    try {
        doom::World world(wad, "e1m1");
        doom::Device dev(W, H);
        dev.upload(world);
        std::FILE *out = std::fopen(argv[4], "wb");
        std::vector<doom::Sector> sectors = world.sectors();
        std::vector<doom::MapObject> objects;
        if ((int)sectors.size() != world.sector_count() || sector < 0 || sector >= (int)sectors.size()) return 3;
        for (int tick = 0; tick < 3; tick++) {
            if (tick == 1) { sectors[(size_t)sector].floor_height = std::atoi(argv[10]); sectors[(size_t)sector].ceiling_height = std::atoi(argv[11]); }
            if (tick == 2) { sectors[(size_t)sector].floor_height = doom::kAsLoaded; sectors[(size_t)sector].ceiling_height = doom::kAsLoaded; }
            doom::sync_state(world, sectors, objects);
            if ((int)world.moved_sectors().size() != (tick == 1 ? 1 : 0)) return 4;
            doom::Pixels pixels(W, H);
            doom::Renderer(pixels, world, pl, 0.0f, dev).render();
            std::fwrite(pixels.pixels.data(), 1, pixels.pixels.size(), out);
        }
        std::fclose(out);
    } catch (const doom::Error &e) { std::fprintf(stderr, "doom::Error %d: %s\n", e.code, e.what()); return 1; }
    return 0;
}
'''


def test_cpp_mirror_with_a_sector_lowered_between_two_renders(tmp_path, dg, oracle, wad1993, path1993, campath_mod, pixel_batch):
    W, H = 320, 200
    c = next(c for c in pixel_batch["cases"] if c.name == "lift")
    (s, fl, ce), = c.entries
    r = path1993[c.frame]
    (tmp_path / "heights.cpp").write_text(MIRROR_SRC)
    (tmp_path / "synth.wad").write_bytes(wad1993)
    exe = tmp_path / "heights"
    lib = os.path.join(ROOT, "doom-rust-renderer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, str(tmp_path / "heights.cpp"), "-o", str(exe), os.path.join(lib, "libdoomgpu.so"), "-Wl,-rpath," + lib])
    run = subprocess.run([str(exe), str(tmp_path / "synth.wad"), str(W), str(H), str(tmp_path / "frames.rgb"), float(r[0]).hex(), float(r[1]).hex(), float(r[2]).hex(),
                          float(r[7]).hex(), str(s), str(fl), str(ce)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    frames = np.fromfile(tmp_path / "frames.rgb", dtype=np.uint8).reshape(3, H, W, 3)
    rec = campath_mod.view_record(np.float32(r[0]), np.float32(r[1]), np.float32(r[2]), np.float32(r[7]))
    plain = sh.oracle_frame(oracle, wad1993, rec, W, H)
    moved = sh.oracle_frame(oracle, c.patched(wad1993), rec, W, H)
    assert np.array_equal(frames[0], plain) and np.array_equal(frames[1], moved) and np.array_equal(frames[2], plain)
    assert not np.array_equal(plain, moved)
