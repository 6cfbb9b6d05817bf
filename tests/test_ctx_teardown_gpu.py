"""GPU tier: destroying a ctx whose work is still queued and whose lazily created streams and events exist (dg_destroy: ~dg_ctx drains
every stream, the owners of hip_mem.hpp then free streams, events and memory), and a dg_create that fails.
1. A ctx with both side streams (dg_reduce_device / dg_reduce_planes_device / dg_seen_lines_device / dg_slot_seen_lines on one,
   dg_ctx_locate_walks on the other) and all four timed intervals, a submission with a dg_readback_async pending in slot 0 and a map
   submission in slot 1, closed without a wait — three times over; a ctx made afterwards renders the same bytes as one made before.
2. dg_create refused for its device ordinal and for its slot count: a dg_create right after each works and renders those bytes.
Only valid calls: nothing here tries to make an allocation fail."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B, SLOTS = 64, 48, 4, 2                              # (map frames need both sides >= 40)
PX = W * H
FRAMES = [0, 297, 500, 728]


@pytest.fixture(scope="module")
def scene(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc
    sc.close()


def _render(dg, scene, views, front_end):
    ctx = dg.Context(W, H, max_batch=B, slots=SLOTS, front_end=front_end)
    ctx.upload_scene(scene)
    out = ctx.render(views).copy()
    ctx.wait(0)
    ctx.close()
    return out


@pytest.mark.parametrize("front_end", [0, 1], ids=["default", "host-lists"])
def test_closing_a_ctx_with_work_queued_and_side_streams_alive(dg, scene, path1993, front_end):
    views = dg.make_views(path1993[FRAMES])
    before = _render(dg, scene, views, front_end)
    words = dg.seen_words(scene)
    slab = B * 3 * PX                                      # a slot's framebuffer slab: the device memory the no-slot calls work in
    seen_at = 16384
    assert words >= 1 and seen_at + B * words * 4 <= slab
    buf = dg.lib().dg_alloc_host(B * 3 * PX)
    assert buf
    walk = dg.Walk(scene, np.full(16, dg.DG_KEY_UP, dtype=np.uint8))
    for _ in range(3):
        ctx = dg.Context(W, H, max_batch=B, slots=SLOTS, front_end=front_end)
        ctx.upload_scene(scene)
        ctx.submit_labels(0, views)                        # slot 0's slab: the id planes (2 B PX bytes), then the class planes
        ctx.wait(0)
        fb0, fb1 = ctx.framebuffer_ptr(0), ctx.framebuffer_ptr(1)
        planes = {"id": fb0, "cls": fb0 + 2 * B * PX}
        ctx.reduce_device(fb0, W, H, B, (2, 2), fb1)       # (B 3 PX bytes read, B 3 PX / 4 written)
        ctx.reduce_planes_device(W, H, B, (2, 2, dg.DG_PLANE_POINT), planes, {"id": fb1, "cls": fb1 + 8192})
        ctx.seen_lines_device(W, H, B, planes["id"], planes["cls"], fb1 + seen_at)
        lines_only = ctx.seen_kernel_ms()
        assert lines_only["accumulate_ms"] == 0.0          # no accumulate kernel ran in that call
        ctx.slot_seen_lines(0, 0, B, B)
        w = dg.Walk(scene, np.full(16, dg.DG_KEY_UP, dtype=np.uint8))
        ctx.locate_walks([w])
        assert np.array_equal(w.floors().view(np.uint32), walk.floors().view(np.uint32))
        w.close()
        # every getter answers DG_OK (the binding raises otherwise): all four intervals exist and are measured
        assert ctx.reduce_kernel_ms() >= 0.0 and ctx.plane_reduce_kernel_ms() >= 0.0
        both = ctx.seen_kernel_ms()
        assert both["lines_ms"] >= 0.0 and both["accumulate_ms"] >= 0.0
        ctx.submit(0, views)
        ctx.readback_async(0, 0, B, buf)
        ctx.submit_map(1, views)
        ctx.close()                                        # neither slot waited for; the copy into buf has run when this returns
    dg.lib().dg_free_host(buf)
    walk.close()
    assert np.array_equal(_render(dg, scene, views, front_end), before)
    # a dg_create that is refused, for its device ordinal and for its slot count, and a good one right after each
    for bad, code in ((dict(device=_device_count()), dg.DG_ERR_NO_DEVICE), (dict(slots=17), dg.DG_ERR_INVALID)):
        with pytest.raises(dg.DoomGpuError) as e:
            dg.Context(W, H, **{**dict(max_batch=B, slots=SLOTS, front_end=front_end), **bad})
        assert e.value.code == code
        assert np.array_equal(_render(dg, scene, views, front_end), before)


def _device_count() -> int:
    """hipGetDeviceCount of the HIP runtime libdoomgpu.so is linked against (the copy this process has loaded)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    n = ctypes.c_int(0)
    assert ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n)) == 0
    return n.value
