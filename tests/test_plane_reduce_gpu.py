"""GPU tier of the reduced depth and label planes, every result byte for byte against the numpy restatement
(np_plane_reduce).
1. dg_reduce_planes_device between torch tensors over the grid the CPU tier runs (64x40 and 320x200 take the 16-byte kernel, 80x50 too;
   131x67, 5x9, 1x1 and a 64x40 source one element off take the any-width one; 16x16 on 5x9 is a box larger than the frame), both rules,
   1, 3 and 65 frames, pairs left out, sentinel elements around every destination.  Every row here, the 1280-wide slot's included,
   is ONE run of dg_plane_nearest (plane_reduce_px_per_wg covers about 2040 source columns), in one launch: rows of several runs, more than 65535 frames and buffers past 2^32 are tests/test_extents_gpu.py's.  These cases, the call's errors and the call with
   slots in flight run in ONE child process (tests/plane_reduce/torch_cases.py), because torch has to be imported before libdoomgpu.so
   is loaded and this session loaded it long ago; the tests here read the child's per-case results.
2. dg_readback_planes_reduced of a bundle, a depth slot and a label slot equals the model applied to dg_readback_depth /
   dg_readback_labels of the same slot, at 320x200 and 1280x800, sub-ranges and count = 0 included; the boxes are dg_readback_labels'.
3. What a slot lacks is refused: NEAREST and depth outputs on a label slot, label outputs on a depth slot, everything on colour.
4. The slot machinery: asynchronous reduced plane readbacks of two slots, one readback in flight per slot of any kind, a new submission,
   dg_upload_scene and dg_wait each complete the pending one, a later request that needs a larger scratch.
5. Every reduced readback leaves the slot's planes as they were."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import np_plane_reduce as npp
import np_reduce as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
ALL = 7
RULES = (npp.POINT, npp.NEAREST)
W0, H0, N0 = 320, 200, 16


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/plane_reduce/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("plane_reduce") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plane_reduce", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_reduce_planes_device_equals_the_model(torch_cases, size, factor):
    assert torch_cases[f"grid/{size[0]}x{size[1]}/{factor[0]}x{factor[1]}"] == "ok"


def test_reduce_planes_device_at_a_base_off_the_16_byte_boundary(torch_cases):
    assert torch_cases["unaligned/64x40"] == "ok"


def test_reduce_planes_device_errors(torch_cases):
    assert torch_cases["errors"] == "ok"


def test_reduce_planes_device_leaves_slots_in_flight_alone(torch_cases):
    assert torch_cases["in_flight"] == "ok"


# ---- the readbacks -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene1993(dg, wad1993):
    sc = dg.Scene(wad1993, "e1m1")
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def views16(dg, path1993):
    return dg.make_views(path1993[0:960:60])


@pytest.fixture(scope="module")
def ctx(dg, scene1993, views16):
    """320x200, max_batch 48, two slots; slot 0 holds a finished bundle of 16 path frames with all three parts."""
    c = dg.Context(W0, H0, max_batch=48, slots=2)
    c.upload_scene(scene1993)
    c.submit_bundle(0, views16, ALL)
    c.wait(0)
    yield c
    c.close()


def _full(c, slot, n, depth=True, labels=True):
    """The slot's full-size planes and boxes through dg_readback_depth / dg_readback_labels: ({name: plane}, boxes or None)."""
    planes, boxes = {}, None
    if depth:
        planes["distance"], planes["kind"] = c.readback_depth(slot, 0, n)
    if labels:
        planes["id"], planes["cls"], boxes = c.readback_labels(slot, 0, n)
    return planes, boxes


def _same_full(a, b):
    assert set(a[0]) == set(b[0]) and all(np.array_equal(a[0][k], b[0][k]) for k in a[0])
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def _same(got, want, boxes, what):
    want = dict(want) if boxes is None else dict(want, boxes=boxes)
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {len(bad)} {k} entries differ, first at {bad[0].tolist()}: gpu {got[k][tuple(bad[0])]} model {want[k][tuple(bad[0])]}"


def check_slot(dg, c, slot, n, depth=True, labels=True):
    """dg_readback_planes_reduced of what the slot holds against the model on its full-size planes: (4,4) and (5,3), the rules the slot
    allows, the whole range and a sub-range, each output alone, count = 0; afterwards the full-size planes are as they were."""
    full = _full(c, slot, n, depth, labels)
    planes, boxes = full
    assert all(a.any() for a in planes.values())
    flags = dict(distance=depth, kind=depth, id=labels, cls=labels, boxes=labels)
    first, count = (1, n - 2) if n > 3 else (1, 2)
    for fx, fy in ((4, 4), (5, 3)):
        for rule in RULES if depth else (npp.POINT,):
            want = npp.reduce(rule, fx, fy, **planes)
            _same(c.readback_planes_reduced(slot, 0, n, (fx, fy, rule), **flags), want, boxes, (fx, fy, rule))
            _same(c.readback_planes_reduced(slot, first, count, (fx, fy, rule), **flags), {k: v[first:first + count] for k, v in want.items()},
                  None if boxes is None else boxes[first:first + count], (fx, fy, rule, "sub-range"))
    want = npp.reduce(RULES[-1] if depth else npp.POINT, 5, 3, **planes)
    for name in [k for k, v in flags.items() if v]:                   # each output alone (NEAREST reads the distance plane whatever is asked for)
        alone = {k: k == name for k in flags}
        got = c.readback_planes_reduced(slot, 0, n, (5, 3, RULES[-1] if depth else npp.POINT), **alone)
        assert list(got) == [name] and np.array_equal(got[name], boxes if name == "boxes" else want[name]), name
    L = dg.lib()
    d = dg.DgPlaneReduceDesc(4, 4, dg.DG_PLANE_POINT, 0)
    one = np.full(64, 0xA5, dtype=np.uint8)
    p = one.ctypes.data_as(P)
    ptrs = [p if flags[k] else None for k in ("distance", "kind", "id", "cls", "boxes")]
    assert L.dg_readback_planes_reduced(c._h, slot, 1, 0, ctypes.byref(d), *ptrs) == dg.DG_OK                  # count = 0
    assert L.dg_readback_planes_reduced(c._h, slot, 0, n, ctypes.byref(d), None, None, None, None, None) == dg.DG_OK    # nothing asked for
    assert (one == 0xA5).all()
    for (f, k) in ((-1, 1), (0, n + 1), (n, 1), (0, -1)):
        assert L.dg_readback_planes_reduced(c._h, slot, f, k, ctypes.byref(d), *ptrs) == dg.DG_ERR_INVALID
        assert L.dg_readback_planes_reduced_async(c._h, slot, f, k, ctypes.byref(d), *ptrs) == dg.DG_ERR_INVALID
    assert (one == 0xA5).all()
    _same_full(_full(c, slot, n, depth, labels), full)                # the planes are left intact
    return full


def test_reduced_planes_of_a_bundle_320x200(dg, ctx):
    planes, boxes = check_slot(dg, ctx, 0, N0)
    assert (boxes["pixels"] > 0).any() and {1, 2, 3} <= set(np.unique(planes["kind"]).tolist())
    near = ctx.readback_planes_reduced(0, 0, N0, (4, 4, npp.NEAREST), boxes=False)
    point = ctx.readback_planes_reduced(0, 0, N0, (4, 4, npp.POINT), boxes=False)
    assert any((near[k] != point[k]).any() for k in npp.NAMES)        # the frames exercise the rule


def test_reduced_planes_of_a_depth_slot_and_a_label_slot(dg, ctx, views16):
    L = dg.lib()
    buf = np.full(2 * W0 * H0 * N0, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(P)
    near, point = dg.DgPlaneReduceDesc(4, 4, dg.DG_PLANE_NEAREST, 0), dg.DgPlaneReduceDesc(4, 4, dg.DG_PLANE_POINT, 0)
    ctx.submit_depth(1, views16)
    check_slot(dg, ctx, 1, N0, labels=False)
    for ptrs in ((None, None, p, None, None), (None, None, None, p, None), (None, None, None, None, p), (p, None, p, None, None)):
        for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
            assert fn(ctx._h, 1, 0, 1, ctypes.byref(near), *ptrs) == dg.DG_ERR_INVALID and b"label" in L.dg_last_error()
    ctx.submit_labels(1, views16)
    check_slot(dg, ctx, 1, N0, depth=False)
    for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
        assert fn(ctx._h, 1, 0, 1, ctypes.byref(near), None, None, p, None, None) == dg.DG_ERR_INVALID and b"NEAREST" in L.dg_last_error()
        assert fn(ctx._h, 1, 0, 1, ctypes.byref(near), None, None, None, None, None) == dg.DG_ERR_INVALID      # (whatever is asked for)
        for ptrs in ((p, None, None, None, None), (None, p, None, None, None), (p, None, p, None, None)):
            assert fn(ctx._h, 1, 0, 1, ctypes.byref(point), *ptrs) == dg.DG_ERR_INVALID and b"depth" in L.dg_last_error()
    # a bundle without one of the parts is ruled on like the slot of the other part
    ctx.submit_bundle(1, views16, dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_LABELS)
    check_slot(dg, ctx, 1, N0, depth=False)
    assert L.dg_readback_planes_reduced(ctx._h, 1, 0, 1, ctypes.byref(point), p, None, None, None, None) == dg.DG_ERR_INVALID
    ctx.submit_bundle(1, views16, dg.DG_BUNDLE_DEPTH)
    check_slot(dg, ctx, 1, N0, labels=False)
    assert (buf == 0xA5).all()
    ctx.wait(1)


def test_colour_slots_are_refused(dg, ctx, views16):
    L = dg.lib()
    buf = np.full(64, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(P)
    point = dg.DgPlaneReduceDesc(4, 4, dg.DG_PLANE_POINT, 0)
    for how in ("colour", "colour bundle"):
        if how == "colour":
            ctx.submit(1, views16)
        else:
            ctx.submit_bundle(1, views16, dg.DG_BUNDLE_COLOUR)
        ctx.wait(1)
        for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
            for ptrs in ((p, None, None, None, None), (None, None, p, None, None), (None, None, None, None, None)):
                assert fn(ctx._h, 1, 0, 1, ctypes.byref(point), *ptrs) == dg.DG_ERR_INVALID, how
        # ... and the colour calls keep refusing plane slots: the colour reduced readback still works on colour
        assert ctx.readback_reduced(1, 0, 1, (4, 4)).shape == (1, 50, 80, 3)
    for bad in (dg.DgPlaneReduceDesc(0, 4, 0, 0), dg.DgPlaneReduceDesc(4, 17, 0, 0), dg.DgPlaneReduceDesc(4, 4, 2, 0), dg.DgPlaneReduceDesc(4, 4, 0, 3)):
        for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
            assert fn(ctx._h, 0, 0, 1, ctypes.byref(bad), p, None, None, None, None) == dg.DG_ERR_INVALID
    for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
        assert fn(ctx._h, 0, 0, 1, None, p, None, None, None, None) == dg.DG_ERR_INVALID
        assert fn(ctx._h, 2, 0, 1, ctypes.byref(point), p, None, None, None, None) == dg.DG_ERR_INVALID        # no such slot
    d = dg.DgReduceDesc(4, 4, 0, 0)
    ctx.submit_depth(1, views16)
    assert L.dg_readback_reduced(ctx._h, 1, 0, 1, ctypes.byref(d), p) == dg.DG_ERR_INVALID                      # as before this feature
    assert L.dg_readback_reduced_async(ctx._h, 1, 0, 1, ctypes.byref(d), p) == dg.DG_ERR_INVALID
    ctx.wait(1)
    assert (buf == 0xA5).all()


def test_reduced_planes_of_a_bundle_1280x800(dg, scene1993, path1993):
    W, H, n = 1280, 800, 3
    c = dg.Context(W, H, max_batch=9, slots=1)
    c.upload_scene(scene1993)
    c.submit_bundle(0, dg.make_views(path1993[[100, 500, 728]]), ALL)
    planes, boxes = _full(c, 0, n)
    for (fx, fy, rule) in ((4, 4, npp.NEAREST), (5, 3, npp.NEAREST), (8, 8, npp.POINT)):
        _same(c.readback_planes_reduced(0, 0, n, (fx, fy, rule)), npp.reduce(rule, fx, fy, **planes), boxes, (fx, fy, rule))
    _same_full(_full(c, 0, n), (planes, boxes))
    c.close()


class Pinned:
    """Page-locked host memory (dg_alloc_host) as one numpy array per output of a reduced plane readback of n frames."""

    def __init__(self, dg, n, oW, oH, n_mobjs):
        self.dg, self.mem, self.arr = dg, {}, {}
        for k in npp.NAMES + ("boxes",):
            dt = np.dtype(dg.LABEL_BOX_DTYPE if k == "boxes" else npp.DTYPES[k])
            shape = (n, n_mobjs) if k == "boxes" else (n, oH, oW)
            nbytes = max(1, int(np.prod(shape)) * dt.itemsize)
            ptr = dg.lib().dg_alloc_host(nbytes)
            assert ptr
            raw = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
            raw[:] = 0xA5
            self.mem[k], self.arr[k] = ptr, raw[:int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape)

    def clear(self):
        for a in self.arr.values():
            a.view(np.uint8)[...] = 0xA5

    def free(self):
        self.arr = None
        for ptr in self.mem.values():
            self.dg.lib().dg_free_host(ptr)


def test_async_reduced_plane_readbacks(dg, scene1993, path1993, views16):
    W, H, n = W0, H0, N0
    L = dg.lib()
    c = dg.Context(W, H, max_batch=48, slots=2)
    c.upload_scene(scene1993)
    n_mobjs = scene1993.mobj_count()
    vb = dg.make_views(path1993[400:400 + n])
    d0, d1 = (8, 8, npp.NEAREST), (5, 3, npp.POINT)
    b0, b1 = Pinned(dg, n, *npp.reduced_size(W, H, 8, 8), n_mobjs), Pinned(dg, 5, *npp.reduced_size(W, H, 5, 3), n_mobjs)
    big = Pinned(dg, n, W, H, n_mobjs)
    plain = dg.lib().dg_alloc_host(n * c.frame_bytes)
    # two slots in flight, each with its reduced readback queued behind its kernels
    c.submit_bundle(0, views16, ALL)
    c.readback_planes_reduced_async(0, 0, n, d0, **b0.mem)
    c.submit_bundle(1, vb, ALL)
    c.readback_planes_reduced_async(1, 2, 5, d1, **b1.mem)
    # one readback in flight per slot, of any kind
    for again in (lambda: c.readback_planes_reduced_async(0, 0, n, d0, **b0.mem), lambda: c.readback_async(0, 0, n, plain),
                  lambda: c.readback_reduced_async(0, 0, n, (4, 4), plain)):
        with pytest.raises(dg.DoomGpuError) as e:
            again()
        assert e.value.code == dg.DG_ERR_INVALID
    c.wait(0)
    c.wait(1)
    full0, full1 = _full(c, 0, n), _full(c, 1, n)
    _same(b0.arr, npp.reduce(d0[2], 8, 8, **full0[0]), full0[1], "slot 0")
    _same(b1.arr, {k: v[2:7] for k, v in npp.reduce(d1[2], 5, 3, **full1[0]).items()}, full1[1][2:7], "slot 1")
    # a reduced plane readback after a plain or a colour-reduced one that is pending
    for first in (lambda: c.readback_async(0, 0, n, plain), lambda: c.readback_reduced_async(0, 0, n, (4, 4), plain)):
        first()
        with pytest.raises(dg.DoomGpuError) as e:
            c.readback_planes_reduced_async(0, 0, n, d0, **b0.mem)
        assert e.value.code == dg.DG_ERR_INVALID
        c.wait(0)
    # dg_wait, a new submission and dg_upload_scene each complete the pending readback first: the host holds the planes of the
    # submission it was queued behind (slot 0: views16), not those of what came after
    want0 = npp.reduce(d0[2], 8, 8, **full0[0])
    for how in ("wait", "submit", "submit_depth", "upload_scene"):
        c.submit_bundle(0, views16, ALL)
        b0.clear()
        c.readback_planes_reduced_async(0, 0, n, d0, **b0.mem)
        if how == "submit":
            c.submit_bundle(0, vb, ALL)
        elif how == "submit_depth":
            c.submit_depth(0, vb)
        elif how == "upload_scene":
            c.upload_scene(scene1993)
        if how != "upload_scene":
            c.wait(0)
        _same(b0.arr, want0, full0[1], how)
    # scratch growth: a small request, then larger ones, synchronous and asynchronous; some outputs only
    c.submit_bundle(0, views16, ALL)
    c.submit_bundle(1, vb, ALL)
    for d in ((16, 16, npp.POINT), (4, 4, npp.NEAREST), (2, 2, npp.NEAREST), (1, 1, npp.NEAREST)):
        _same(c.readback_planes_reduced(0, 0, n, d), npp.reduce(d[2], d[0], d[1], **full0[0]), full0[1], d)
        oW, oH = npp.reduced_size(W, H, d[0], d[1])
        big.clear()
        c.readback_planes_reduced_async(1, 0, n, d, distance=big.mem["distance"], cls=big.mem["cls"], boxes=big.mem["boxes"])
        # a synchronous reduced readback of the same slot completes the pending one first (they share the scratch)
        _same(c.readback_planes_reduced(1, 3, 2, (8, 8, npp.POINT), boxes=False), {k: v[3:5] for k, v in npp.reduce(npp.POINT, 8, 8, **full1[0]).items()}, None, d)
        assert L.dg_readback_planes_reduced_async(c._h, 1, 0, 1, ctypes.byref(dg.DgPlaneReduceDesc(8, 8, 0, 0)), None, None, None, None, None) == dg.DG_OK
        want = npp.reduce(d[2], d[0], d[1], **full1[0])
        for k in ("distance", "cls"):
            got = big.arr[k].reshape(-1)[:n * oW * oH].reshape(n, oH, oW)
            assert np.array_equal(got, want[k]), (d, k)
        assert np.array_equal(big.arr["boxes"], full1[1])
        assert (big.arr["kind"].view(np.uint8) == 0xA5).all() and (big.arr["id"].view(np.uint8) == 0xA5).all()
    c.wait(1)
    _same_full(_full(c, 0, n), full0)
    _same_full(_full(c, 1, n), full1)
    for b in (b0, b1, big):
        b.free()
    dg.lib().dg_free_host(plain)
    c.close()
