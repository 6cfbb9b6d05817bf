"""GPU tier of the screen pictures: dg_overlay_device on torch buffers (one child process,
tests/overlay/torch_cases.py: torch has to be imported before libdoomgpu.so is loaded) and dg_slot_overlay on the frames of a slot,
every pixel of every frame against dg_overlay_host applied to the frames as they were rendered.

  device     every case list of overlay_cases at 131x67 and 64x48, and the screen of tools/overlay_bench.py at 1280x800 on 3 frames:
             against dg_overlay_host and np_overlay, with sentinels around the frames
  slot       after a submission through each front end, caller-built lists and the three 2-D map submissions at 131x67: frames 1..3 of 5
             carry the pictures, frames 0 and 4 are the plain render; dg_frame_checksums and dg_readback_reduced see the overlaid frames; a
             bundle with colour at its offset; a bundle without colour and a depth slot are refused
  redone     a column-walk batch that overflows: dg_slot_overlay makes the submission final first, the redone frame carries the pictures
  pending    refused while dg_readback_async is pending, accepted after dg_wait
  late       a picture loaded after dg_upload_scene is refused until the scene is uploaded again
  big        1280x800 frames just over 4 GiB
  time       dg_ctx_overlay_kernel_ms errors before the first launch and is > 0 after it
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import np_reduce as npr
import overlay_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 131, 67, 5
CASE_IDS = [f"{w}x{h}/{name}" for (w, h) in oc.SIZES for name in oc.cases(w, h)]
CHILD_SECONDS = 300


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/overlay/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("overlay") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlay", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=CHILD_SECONDS)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


@pytest.mark.parametrize("case", CASE_IDS)
def test_overlay_device_case_by_case(torch_cases, case):
    assert torch_cases[f"cases/{case}"] == "ok"


def test_overlay_device_the_screen_at_1280x800(torch_cases):
    assert torch_cases["hud/1280x800"] == "ok"


def test_overlay_device_past_4_gib(torch_cases):
    result = torch_cases["big/past 4 GiB"]
    if result.startswith("out of memory"):
        pytest.skip(result[:300])
    assert result == "ok"


@pytest.fixture(scope="module")
def scene(dg):
    s = oc.load(dg)
    yield s
    s.close()


@pytest.fixture(scope="module")
def views(dg, path1993):
    return dg.make_views(path1993[[100, 300, 500, 728, 900]])


def items3():
    c = oc.cases(W, H)
    return [c["two and three overlapping, holes on top"][2], [], c["clipped by two edges at once"][0] + oc.hud(W, H)]


def same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first (frame, y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def overlaid(dg, scene, base, items, first=1):
    want = base.copy()
    dg.overlay_host(scene, want[first:first + len(items)], items)
    return want


def check_slot(dg, scene, ctx, what):
    """The slot's frames as rendered, then dg_slot_overlay on frames 1..3, then what every reader of the slot sees."""
    base = ctx.readback(0, 0, N).copy()
    ctx.slot_overlay(0, 1, items3())
    want = overlaid(dg, scene, base, items3())
    same(ctx.readback(0, 0, N), want, what)
    assert (want[1] != base[1]).any() and (want[3] != base[3]).any() and (want[2] == base[2]).all()
    assert ctx.frame_checksums(0, 0, N).tolist() == [dg.frame_checksum(f) for f in want], what
    assert np.array_equal(ctx.readback_reduced(0, 0, N, (2, 2)), npr.reduce(want, 2, 2, npr.RGB24)), what
    assert ctx.overlay_kernel_ms() > 0.0


SUBMISSIONS = ["host", "device", "device_segs", "lists", "map", "explored", "ego"]


@pytest.mark.parametrize("how", SUBMISSIONS)
def test_slot_overlay_after_every_kind_of_colour_submission(dg, scene, views, how):
    fe = {"host": dg.DG_FE_HOST, "device": dg.DG_FE_DEVICE, "device_segs": dg.DG_FE_DEVICE_SEGS}.get(how, dg.DG_FE_HOST)
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=fe)
    ctx.upload_scene(scene)
    if how in ("host", "device", "device_segs"):
        ctx.submit(0, views)
    elif how == "lists":
        fl = scene.build_lists(W, H, views[2])
        ctx.draw_lists(0, (dg.DgFrameLists * N)(*([fl] * N)))
    elif how == "map":
        ctx.submit_map(0, views)
    elif how == "explored":
        ctx.submit_explored_map(0, views, np.full((N, dg.seen_words(scene)), 0xFFFFFFFF, np.uint32))
    else:
        ctx.submit_ego_map(0, views, (1.0, 0))
    check_slot(dg, scene, ctx, how)
    # twice draws twice (the same pixels); a replay renders over the pictures
    if how in ("host", "device", "device_segs"):
        after = ctx.readback(0, 0, N).copy()
        ctx.slot_overlay(0, 1, items3())
        same(ctx.readback(0, 0, N), after, (how, "twice"))
        ctx.replay(0)
        same(ctx.readback(0, 0, N), ctx.render(views), (how, "replay"))
    ctx.close()


def test_slot_overlay_on_bundles_and_refusals(dg, scene, views):
    L = dg.lib()
    ctx = dg.Context(W, H, max_batch=4 * N, slots=1)
    ctx.upload_scene(scene)
    items, first = dg.screen_pictures(items3())
    ip, fp = items.ctypes.data_as(ctypes.c_void_p), first.ctypes.data_as(ctypes.c_void_p)
    assert L.dg_slot_overlay(ctx._h, 0, 0, 0, ip, fp) == dg.DG_OK                      # an empty slot, no frames: nothing to do
    assert L.dg_slot_overlay(ctx._h, 0, 0, 1, ip, fp) == dg.DG_ERR_INVALID
    ctx.submit_bundle(0, views, 7)                                             # colour, depth, labels: the colour part at its offset
    depth = ctx.readback_depth(0, 0, N)
    check_slot(dg, scene, ctx, "bundle 7")
    for a, b in zip(depth, ctx.readback_depth(0, 0, N)):
        assert np.array_equal(a, b)                                            # (the planes next to the frames are not touched)
    ctx.submit_bundle(0, views, 5)
    check_slot(dg, scene, ctx, "bundle 5")
    for (f0, cnt) in ((-1, 3), (3, 3), (0, N + 1), (0, -1)):                   # a bad frame range
        assert L.dg_slot_overlay(ctx._h, 0, f0, cnt, ip, fp) == dg.DG_ERR_INVALID, (f0, cnt)
    assert L.dg_slot_overlay(ctx._h, 1, 1, 3, ip, fp) == dg.DG_ERR_INVALID and L.dg_slot_overlay(ctx._h, -1, 1, 3, ip, fp) == dg.DG_ERR_INVALID
    bad, bfirst = dg.screen_pictures([[(scene.picture_count(), 0, 0)], [], []])
    before = ctx.readback(0, 0, N).copy()
    assert L.dg_slot_overlay(ctx._h, 0, 1, 3, bad.ctypes.data_as(ctypes.c_void_p), bfirst.ctypes.data_as(ctypes.c_void_p)) == dg.DG_ERR_INVALID
    same(ctx.readback(0, 0, N), before, "a refused call draws nothing")
    ctx.submit_bundle(0, views, 6)                                             # no colour part
    assert L.dg_slot_overlay(ctx._h, 0, 1, 3, ip, fp) == dg.DG_ERR_INVALID and b"colour" in L.dg_last_error()
    ctx.submit_depth(0, views)
    planes = [p.copy() for p in ctx.readback_depth(0, 0, N)]
    assert L.dg_slot_overlay(ctx._h, 0, 1, 3, ip, fp) == dg.DG_ERR_INVALID
    for a, b in zip(planes, ctx.readback_depth(0, 0, N)):
        assert np.array_equal(a, b)
    ctx.submit_labels(0, views)
    assert L.dg_slot_overlay(ctx._h, 0, 1, 3, ip, fp) == dg.DG_ERR_INVALID
    ctx.close()


def test_a_redone_frame_carries_the_pictures(dg, scene, views, monkeypatch):
    """DOOMGPU_FE_COLUMN_SLOTS=3 makes the device column walk overflow; dg_slot_overlay comes before any wait, so it is the call that
    makes the submission final (frames redone on the host) before it draws."""
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "3")
    ctx = dg.Context(W, H, max_batch=N, slots=1, front_end=dg.DG_FE_DEVICE)
    ctx.upload_scene(scene)
    ctx.submit(0, views)
    ctx.slot_overlay(0, 1, items3())
    counts = ctx.fallbacks()
    assert counts["front_end"] > 0 and counts["redone_frames"] > 0, counts
    got = ctx.readback(0, 0, N)
    monkeypatch.delenv("DOOMGPU_FE_COLUMN_SLOTS")
    plain = dg.Context(W, H, max_batch=N, slots=1, front_end=dg.DG_FE_HOST)
    plain.upload_scene(scene)
    same(got, overlaid(dg, scene, plain.render(views), items3()), "redone")
    plain.close()
    ctx.close()


def test_refused_while_an_asynchronous_readback_is_pending(dg, scene, views):
    L = dg.lib()
    ctx = dg.Context(W, H, max_batch=N, slots=1)
    ctx.upload_scene(scene)
    host = L.dg_alloc_host(N * ctx.frame_bytes)
    assert host
    try:
        ctx.submit(0, views)
        ctx.readback_async(0, 0, N, host)
        items, first = dg.screen_pictures(items3())
        assert L.dg_slot_overlay(ctx._h, 0, 1, 3, items.ctypes.data_as(ctypes.c_void_p), first.ctypes.data_as(ctypes.c_void_p)) == dg.DG_ERR_INVALID
        assert b"pending" in L.dg_last_error()
        ctx.wait(0)
        base = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint8)), shape=(N, H, W, 3)).copy()
        same(ctx.readback(0, 0, N), base, "the refused call drew nothing, and the copy got the frames as rendered")
        ctx.slot_overlay(0, 1, items3())
        same(ctx.readback(0, 0, N), overlaid(dg, scene, base, items3()), "after dg_wait")
    finally:
        ctx.close()
        L.dg_free_host(host)


def test_a_picture_loaded_after_the_upload_is_refused_until_the_next(dg, views):
    L = dg.lib()
    scene = dg.Scene(oc.wad(), "e1m1")
    assert scene.use_picture("BON1A0") == 0
    ctx = dg.Context(W, H, max_batch=N, slots=1)
    with pytest.raises(dg.DoomGpuError):
        ctx.overlay_kernel_ms()                                                # nothing launched yet
    items, first = dg.screen_pictures([[(0, 3, 3, 2, 2)], [], []])
    ip, fp = items.ctypes.data_as(ctypes.c_void_p), first.ctypes.data_as(ctypes.c_void_p)
    assert L.dg_slot_overlay(ctx._h, 0, 0, 0, ip, fp) == dg.DG_ERR_INVALID and L.dg_overlay_device(ctx._h, ctypes.c_void_p(64), W, H, 3, ip, fp) == dg.DG_ERR_INVALID   # no scene
    ctx.upload_scene(scene)
    ctx.submit(0, views)
    ctx.wait(0)
    with pytest.raises(dg.DoomGpuError):
        ctx.overlay_kernel_ms()
    late = scene.use_picture("XHAIR")
    assert late == 1
    with pytest.raises(dg.DoomGpuError) as e:
        ctx.slot_overlay(0, 1, [[(late, 60, 30, 3, 3)], [], []])
    assert e.value.code == dg.DG_ERR_INVALID
    base = ctx.readback(0, 0, N).copy()
    ctx.slot_overlay(0, 1, [[(0, 3, 3, 2, 2)], [], []])                       # what the uploaded copy holds still draws
    same(ctx.readback(0, 0, N), overlaid(dg, scene, base, [[(0, 3, 3, 2, 2)], [], []]), "the uploaded picture")
    assert ctx.overlay_kernel_ms() > 0.0
    ctx.upload_scene(scene)
    ctx.submit(0, views)
    base = ctx.readback(0, 0, N).copy()
    ctx.slot_overlay(0, 1, [[(late, 60, 30, 3, 3)], [], [(0, 1, 1)]])
    same(ctx.readback(0, 0, N), overlaid(dg, scene, base, [[(late, 60, 30, 3, 3)], [], [(0, 1, 1)]]), "after the second upload")
    ctx.close()
    scene.close()
