"""The eight readback calls of one slot next to each other (api_readback.cpp), where the other GPU tests take them one at a time.
320x200, one slot, four path frames of e1m1 as a bundle with all three parts; max_batch 12 is the smallest whose framebuffer slab holds
the nine bytes per pixel of four such views (dg_bundle_capacity).
1. Under a pending dg_readback_planes_reduced_async with boxes, which owns the slot's scratch and box staging until dg_wait, the
   full-size calls (dg_readback_labels with boxes, dg_readback_depth, dg_readback) and dg_frame_checksums give what they give on the
   settled slot, and the pending one's outputs are the model's (np_plane_reduce) on the full-size planes, its boxes the full-size boxes.
2. Under a pending dg_readback_reduced_async, a dg_readback_reduced with another factor and a dg_readback_planes_reduced, which both
   need the scratch it owns, are right, and so are the pending one's bytes after dg_wait.
3. Every bad frame range is refused by all eight calls with DG_ERR_INVALID, writes nothing, leaves nothing pending and leaves the slot
   able to deliver its frames."""
import ctypes

import numpy as np
import pytest

import np_plane_reduce as npp
from test_plane_reduce_gpu import Pinned

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
W, H, N = 320, 200, 4
ALL = 7


@pytest.fixture(scope="module")
def slot(dg, wad1993, path1993):
    """(ctx, views, what the settled slot 0 holds: frames, checksums, {plane name: plane}, boxes)."""
    sc = dg.Scene(wad1993, "e1m1")
    c = dg.Context(W, H, max_batch=12, slots=1)
    c.upload_scene(sc)
    views = dg.make_views(path1993[0:960:240])
    c.submit_bundle(0, views, ALL)
    c.wait(0)
    planes = {}
    planes["distance"], planes["kind"] = c.readback_depth(0, 0, N)
    planes["id"], planes["cls"], boxes = c.readback_labels(0, 0, N)
    settled = dict(frames=c.readback(0, 0, N), sums=c.frame_checksums(0, 0, N), planes=planes, boxes=boxes)
    assert settled["frames"].any() and all(a.any() for a in planes.values()) and (boxes["pixels"] > 0).any()
    yield c, views, settled
    c.close()
    sc.close()


def _same_planes(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def test_full_size_readbacks_under_a_pending_reduced_plane_readback(dg, slot):
    c, views, settled = slot
    desc = (5, 3, npp.NEAREST)
    pending = Pinned(dg, N, *npp.reduced_size(W, H, 5, 3), settled["boxes"].shape[1])
    c.submit_bundle(0, views, ALL)
    c.readback_planes_reduced_async(0, 0, N, desc, **pending.mem)
    ident, cls, boxes = c.readback_labels(0, 0, N)
    distance, kind = c.readback_depth(0, 0, N)
    frames = c.readback(0, 0, N)
    sums = c.frame_checksums(0, 0, N)
    with pytest.raises(dg.DoomGpuError):                              # (it is still pending: none of them completed it)
        c.readback_planes_reduced_async(0, 0, N, desc, **pending.mem)
    c.wait(0)
    _same_planes(dict(distance=distance, kind=kind, id=ident, cls=cls), settled["planes"], "synchronous")
    assert np.array_equal(boxes, settled["boxes"]) and np.array_equal(frames, settled["frames"]) and np.array_equal(sums, settled["sums"])
    _same_planes(pending.arr, npp.reduce(desc[2], 5, 3, **settled["planes"]), "pending")
    assert np.array_equal(pending.arr["boxes"], settled["boxes"])
    pending.free()


def test_reduced_readbacks_under_a_pending_reduced_frame_readback(dg, slot):
    c, views, settled = slot
    L = dg.lib()
    want = dg.reduce_host(settled["frames"], (4, 4))
    mem = L.dg_alloc_host(want.nbytes)
    assert mem
    pending = np.ctypeslib.as_array(ctypes.cast(mem, ctypes.POINTER(ctypes.c_uint8)), shape=(want.nbytes,))
    pending[:] = 0xA5
    c.submit_bundle(0, views, ALL)
    c.readback_reduced_async(0, 0, N, (4, 4), mem)
    other = c.readback_reduced(0, 1, 2, (5, 3))
    got = c.readback_planes_reduced(0, 0, N, (4, 4, npp.NEAREST))
    c.wait(0)
    assert np.array_equal(other, dg.reduce_host(settled["frames"][1:3], (5, 3)))
    _same_planes(got, npp.reduce(npp.NEAREST, 4, 4, **settled["planes"]), "planes")
    assert np.array_equal(got["boxes"], settled["boxes"])
    assert np.array_equal(pending.reshape(want.shape), want)
    del pending
    L.dg_free_host(mem)


def test_every_call_refuses_every_bad_range(dg, slot):
    c, views, settled = slot
    L, h = dg.lib(), c._h
    # (room for N + 1 frames of the widest output: a range that slipped through would stay inside the buffers)
    bufs = [np.full((N + 1) * W * H * 3, 0xA5, dtype=np.uint8) for _ in range(4)]
    bufs.append(np.full((N + 1) * settled["boxes"].shape[1] * dg.LABEL_BOX_DTYPE.itemsize + 1, 0xA5, dtype=np.uint8))
    a, b, c2, d2, bx = [x.ctypes.data_as(P) for x in bufs]
    rd, pd = dg.DgReduceDesc(4, 4, 0, 0), dg.DgPlaneReduceDesc(4, 4, dg.DG_PLANE_NEAREST, 0)
    calls = {
        "dg_readback": lambda f, k: L.dg_readback(h, 0, f, k, a),
        "dg_readback_async": lambda f, k: L.dg_readback_async(h, 0, f, k, a),
        "dg_readback_reduced": lambda f, k: L.dg_readback_reduced(h, 0, f, k, ctypes.byref(rd), a),
        "dg_readback_reduced_async": lambda f, k: L.dg_readback_reduced_async(h, 0, f, k, ctypes.byref(rd), a),
        "dg_readback_depth": lambda f, k: L.dg_readback_depth(h, 0, f, k, a, b),
        "dg_readback_labels": lambda f, k: L.dg_readback_labels(h, 0, f, k, a, b, bx),
        "dg_readback_planes_reduced": lambda f, k: L.dg_readback_planes_reduced(h, 0, f, k, ctypes.byref(pd), a, b, c2, d2, bx),
        "dg_readback_planes_reduced_async": lambda f, k: L.dg_readback_planes_reduced_async(h, 0, f, k, ctypes.byref(pd), a, b, c2, d2, bx),
    }
    c.submit_bundle(0, views, ALL)
    for name, call in calls.items():
        for f, k in ((-1, 1), (0, N + 1), (N, 1), (0, -1)):
            assert call(f, k) == dg.DG_ERR_INVALID, (name, f, k)
    assert all((x == 0xA5).all() for x in bufs)
    assert L.dg_readback_async(h, 0, 0, 1, a) == dg.DG_OK             # nothing was left pending
    c.wait(0)
    assert np.array_equal(bufs[0][:W * H * 3].reshape(H, W, 3), settled["frames"][0])
    assert np.array_equal(c.readback(0, 0, N), settled["frames"])
