"""GPU tier of the reduced-size frames, every result byte for byte against the numpy restatement (np_reduce).
1. dg_reduce_device between torch uint8 tensors over the grid the CPU tier runs (64x40, 80x50 and 320x200 take the 16-byte kernel:
   their rows are 192, 240 and 960 bytes; 131x67, 5x9 and 1x1 the any-width one; 16x16 on 5x9 is a box larger than the frame), 1, 3
   and 65 frames, a source and a destination offset by one byte, and sentinel bytes around the destination.  Every row here, the
   1280-wide slot's included, is ONE run of its kernel (reduce_px_per_wg covers about 1360 source pixels), one launch, and far below
   2^32 bytes: rows of several runs, more than 65535 frames and buffers past 2^32 are tests/test_extents_gpu.py's.  These cases, the slot's framebuffer reduced into a tensor and
   dg_reduce_device with slots in flight run in ONE child process (tests/reduce/torch_cases.py), because torch has to be imported
   before libdoomgpu.so is loaded and this session loaded it long ago; the tests here read the child's per-case results.
2. dg_readback_reduced of rendered frames equals the model applied to dg_readback, at 320x200 and 1280x800, sub-ranges included.
3. The slot machinery: asynchronous reduced readbacks of two slots, one readback in flight per slot (plain or reduced), a slot
   rendered into again completes its pending reduced readback first, a later descriptor that needs a larger scratch.
4. Frames redone after a capacity overflow (DOOMGPU_FE_COLUMN_SLOTS=5, the project's normal fallback) reach a reduced readback that was
   queued before dg_wait.
5. A reduced readback leaves the slot's frames as they were."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import np_reduce as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/reduce/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("reduce") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reduce", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


@pytest.fixture(scope="module")
def scene1993(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def ctx(dg, scene1993, path1993):
    """320x200, 16 frames of path1993 rendered into slot 0 and finished."""
    c = dg.Context(320, 200, max_batch=16, slots=2)
    c.upload_scene(scene1993)
    c.submit(0, dg.make_views(path1993[0:960:60]))
    c.wait(0)
    yield c
    c.close()


class Pinned:
    """Page-locked host bytes (dg_alloc_host) as a numpy array."""

    def __init__(self, dg, n):
        self.dg, self.ptr = dg, dg.lib().dg_alloc_host(n)
        assert self.ptr
        self.arr = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))
        self.arr[:] = 0xA5

    def free(self):
        self.arr = None
        self.dg.lib().dg_free_host(self.ptr)


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_reduce_device_equals_the_model(torch_cases, size, factor):
    assert torch_cases[f"grid/{size[0]}x{size[1]}/{factor[0]}x{factor[1]}"] == "ok"


@pytest.mark.parametrize("size", [(64, 40), (131, 67), (320, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reduce_device_at_an_unaligned_base(torch_cases, size):
    assert torch_cases[f"unaligned/{size[0]}x{size[1]}"] == "ok"


def test_reduce_device_from_a_slot_framebuffer_into_a_tensor(torch_cases):
    assert torch_cases["framebuffer"] == "ok"


def test_reduce_device_leaves_a_slot_in_flight_alone(torch_cases):
    assert torch_cases["in_flight"] == "ok"


class _DevicePtr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_reduce_device_errors(dg, ctx):
    L = dg.lib()
    t = _DevicePtr(ctx.framebuffer_ptr(1))               # device memory of the ctx; no call below gets as far as touching it
    ok = dg.DgReduceDesc(2, 2, 0, 0)
    P = ctypes.c_void_p
    assert L.dg_reduce_device(ctx._h, P(t.data_ptr()), 8, 8, 0, ctypes.byref(ok), P(t.data_ptr() + 2048)) == dg.DG_OK
    for args in ((None, 8, 8, 1, ctypes.byref(ok), P(t.data_ptr())), (P(t.data_ptr()), 8, 8, 1, ctypes.byref(ok), None),
                 (P(t.data_ptr()), 8, 8, 1, None, P(t.data_ptr())), (P(t.data_ptr()), 0, 8, 1, ctypes.byref(ok), P(t.data_ptr())),
                 (P(t.data_ptr()), 8, 16385, 1, ctypes.byref(ok), P(t.data_ptr())), (P(t.data_ptr()), 8, 8, -1, ctypes.byref(ok), P(t.data_ptr()))):
        assert L.dg_reduce_device(ctx._h, *args) == dg.DG_ERR_INVALID
    for d in (dg.DgReduceDesc(0, 2, 0, 0), dg.DgReduceDesc(2, 17, 0, 0), dg.DgReduceDesc(2, 2, 2, 0), dg.DgReduceDesc(2, 2, 0, 7)):
        assert L.dg_reduce_device(ctx._h, P(t.data_ptr()), 8, 8, 1, ctypes.byref(d), P(t.data_ptr() + 2048)) == dg.DG_ERR_INVALID
        assert L.dg_readback_reduced(ctx._h, 0, 0, 1, ctypes.byref(d), P(t.data_ptr())) == dg.DG_ERR_INVALID
        assert L.dg_readback_reduced_async(ctx._h, 0, 0, 1, ctypes.byref(d), P(t.data_ptr())) == dg.DG_ERR_INVALID
    host = np.zeros(16, dtype=np.uint8)
    hp = host.ctypes.data_as(P)
    for fn in (L.dg_readback_reduced, L.dg_readback_reduced_async):
        assert fn(ctx._h, 0, 0, 1, None, hp) == dg.DG_ERR_INVALID
        assert fn(ctx._h, 0, 0, 1, ctypes.byref(ok), None) == dg.DG_ERR_INVALID
        assert fn(ctx._h, 0, 10, 7, ctypes.byref(ok), hp) == dg.DG_ERR_INVALID          # the slot holds 16 frames
        assert fn(ctx._h, 0, -1, 1, ctypes.byref(ok), hp) == dg.DG_ERR_INVALID
        assert fn(ctx._h, 9, 0, 1, ctypes.byref(ok), hp) == dg.DG_ERR_INVALID           # no such slot
    assert not host.any()


def check_rendered(dg, c, n):
    full = c.readback(0, 0, n)
    sums = c.frame_checksums(0, 0, n)
    for fx, fy in ((4, 4), (5, 3)):
        for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
            want = npr.reduce(full, fx, fy, fmt)
            assert np.array_equal(c.readback_reduced(0, 0, n, (fx, fy, fmt)), want), (fx, fy, fmt)
            first, count = (1, n - 2) if n > 3 else (1, 2)
            assert np.array_equal(c.readback_reduced(0, first, count, (fx, fy, fmt)), want[first:first + count]), (fx, fy, fmt, "sub-range")
    d = dg.DgReduceDesc(4, 4, 0, 0)
    one = np.full(8, 0xA5, dtype=np.uint8)
    assert dg.lib().dg_readback_reduced(c._h, 0, 1, 0, ctypes.byref(d), one.ctypes.data_as(ctypes.c_void_p)) == dg.DG_OK    # count = 0
    assert (one == 0xA5).all()
    assert np.array_equal(c.frame_checksums(0, 0, n), sums) and np.array_equal(c.readback(0, 0, n), full)    # the frames are as they were


def test_readback_reduced_of_rendered_frames_320x200(dg, ctx):
    assert ctx.readback(0, 0, 16).any()
    check_rendered(dg, ctx, 16)


def test_readback_reduced_of_rendered_frames_1280x800(dg, scene1993, path1993):
    c = dg.Context(1280, 800, max_batch=3, slots=1)
    c.upload_scene(scene1993)
    c.submit(0, dg.make_views(path1993[[100, 500, 728]]))
    check_rendered(dg, c, 3)
    c.close()


def test_async_reduced_readbacks_of_two_slots(dg, scene1993, path1993):
    W, H, B = 320, 200, 16
    c = dg.Context(W, H, max_batch=B, slots=2)
    c.upload_scene(scene1993)
    va, vb = dg.make_views(path1993[0:B]), dg.make_views(path1993[400:400 + B])
    d0, d1 = (4, 4, dg.DG_REDUCE_RGB24), (5, 3, dg.DG_REDUCE_GRAY8)
    b0, b1 = Pinned(dg, B * npr.reduced_size(W, H, *d0)[2]), Pinned(dg, 5 * npr.reduced_size(W, H, *d1)[2])
    plain = Pinned(dg, B * c.frame_bytes)
    c.submit(0, va)
    c.readback_reduced_async(0, 0, B, d0, b0.ptr)
    c.submit(1, vb)
    c.readback_reduced_async(1, 2, 5, d1, b1.ptr)
    for again in (lambda: c.readback_async(0, 0, B, plain.ptr), lambda: c.readback_reduced_async(0, 0, B, d0, b0.ptr)):
        with pytest.raises(dg.DoomGpuError) as e:             # one readback in flight per slot: plain after reduced, reduced after reduced
            again()
        assert e.value.code == dg.DG_ERR_INVALID
    c.wait(0)
    c.wait(1)
    assert np.array_equal(b0.arr, npr.reduce(c.readback(0, 0, B), *d0).reshape(-1))
    assert np.array_equal(b1.arr, npr.reduce(c.readback(1, 2, 5), *d1).reshape(-1))
    # reduced after plain
    c.submit(0, vb)
    c.readback_async(0, 0, B, plain.ptr)
    with pytest.raises(dg.DoomGpuError) as e:
        c.readback_reduced_async(0, 0, B, d0, b0.ptr)
    assert e.value.code == dg.DG_ERR_INVALID
    c.wait(0)
    assert np.array_equal(plain.arr, c.readback(0, 0, B).reshape(-1))
    # a descriptor that needs more scratch than the slot has, after smaller ones; synchronous and asynchronous
    full = c.readback(0, 0, B)
    for d in ((8, 8, dg.DG_REDUCE_GRAY8), (4, 4, dg.DG_REDUCE_RGB24), (2, 2, dg.DG_REDUCE_RGB24), (1, 1, dg.DG_REDUCE_RGB24)):
        assert np.array_equal(c.readback_reduced(0, 0, B, d), npr.reduce(full, *d)), d
    full1 = c.readback(1, 0, B)
    for d in ((16, 16, dg.DG_REDUCE_GRAY8), (2, 2, dg.DG_REDUCE_RGB24), (1, 1, dg.DG_REDUCE_RGB24)):
        c.readback_reduced_async(1, 0, B, d, plain.ptr)
        c.wait(1)
        n = B * npr.reduced_size(W, H, *d)[2]
        assert np.array_equal(plain.arr[:n], npr.reduce(full1, *d).reshape(-1)), d
    for b in (b0, b1, plain):
        b.free()
    c.close()


def test_rerendering_a_slot_completes_its_pending_readback_first(dg, scene1993, path1993):
    """A dg_readback_reduced_async still pending when the slot is rendered into again — dg_replay_slot, dg_prepare_views with OTHER
    views, dg_upload_scene — is completed first: the host buffer holds the reduced frames of the submission it was queued behind."""
    W, H, B = 1280, 800, 24
    d = (2, 2, dg.DG_REDUCE_RGB24)
    c = dg.Context(W, H, max_batch=B, slots=1)
    c.upload_scene(scene1993)
    va, vb = dg.make_views(path1993[0:B]), dg.make_views(path1993[500:500 + B])
    want = npr.reduce(c.render(va), *d).reshape(-1)
    buf = Pinned(dg, want.size)
    for how in ("prepare+replay", "replay", "upload_scene", "submit"):
        c.submit(0, va)
        buf.arr[:] = 0
        c.readback_reduced_async(0, 0, B, d, buf.ptr)
        if how == "prepare+replay":
            c.prepare(0, vb)                                   # different frames into the same framebuffer
            c.replay(0)
        elif how == "replay":
            c.replay(0)
        elif how == "upload_scene":
            c.upload_scene(scene1993)
        else:
            c.submit(0, vb)
        c.wait(0)
        assert np.array_equal(buf.arr, want), how
    buf.free()
    c.close()


def test_redone_frames_reach_a_queued_reduced_readback(dg, wad1994, path1994, monkeypatch):
    """The overflow of test_device_front_end_capacity_falls_back_to_host_lists: frames that exceed the column scratch are redone at
    dg_wait, after the reduced readback queued behind the batch has run once.  It is issued again: the host holds the final frames'."""
    W, H = 320, 200
    idx = list(range(0, 1000, 50))
    n = len(idx)
    sc = dg.Scene(wad1994, "e1m1")
    monkeypatch.setenv("DOOMGPU_FE_COLUMN_SLOTS", "5")
    c = dg.Context(W, H, max_batch=n, slots=2, front_end=dg.DG_FE_DEVICE)
    monkeypatch.delenv("DOOMGPU_FE_COLUMN_SLOTS")
    c.upload_scene(sc)
    views = dg.make_views(path1994[idx])
    for d in ((4, 4, dg.DG_REDUCE_RGB24), (5, 3, dg.DG_REDUCE_GRAY8)):
        before = c.fallbacks()
        buf = Pinned(dg, n * npr.reduced_size(W, H, *d)[2])
        c.submit(0, views)
        c.readback_reduced_async(0, 0, n, d, buf.ptr)
        c.wait(0)
        after = c.fallbacks()
        assert after["front_end"] == before["front_end"] + 1 and after["redone_frames"] > before["redone_frames"], (before, after)
        assert c.timing(0)["front_end"] == dg.DG_FE_DEVICE
        final = c.readback(0, 0, n)
        assert np.array_equal(buf.arr, npr.reduce(final, *d).reshape(-1)), d
        buf.free()
    # (the final frames are those of the host list path)
    host = dg.Context(W, H, max_batch=n, slots=1, front_end=dg.DG_FE_HOST)
    host.upload_scene(sc)
    assert np.array_equal(host.render(views), final)
    host.close()
    c.close()
    sc.close()


def test_a_reduced_readback_leaves_the_frames_as_they_were(dg, scene1993, path1993):
    W, H, B = 640, 400, 64
    c = dg.Context(W, H, max_batch=B, slots=2)
    c.upload_scene(scene1993)
    want = c.render(dg.make_views(path1993[0:B])).copy()
    sums = c.frame_checksums(0, 0, B)
    buf = Pinned(dg, B * npr.reduced_size(W, H, 4, 4, npr.GRAY8)[2])
    assert np.array_equal(c.readback_reduced(0, 0, B, (4, 4)), npr.reduce(want, 4, 4))
    c.readback_reduced_async(0, 0, B, (4, 4, dg.DG_REDUCE_GRAY8), buf.ptr)
    c.wait(0)
    assert np.array_equal(buf.arr, npr.reduce(want, 4, 4, npr.GRAY8).reshape(-1))
    assert np.array_equal(c.frame_checksums(0, 0, B), sums) and np.array_equal(c.readback(0, 0, B), want)
    buf.free()
    c.close()
