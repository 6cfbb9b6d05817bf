"""torch_cases.py OUT.json — the cases of tests/test_explored_gpu.py that hand torch tensors to dg_seen_lines_device, run in a process of
their own: a torch wheel that brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded, so that both resolve the one
runtime; in a pytest session the library is long loaded.  Every case is compared with the numpy restatement
(np_explored) here; OUT.json maps a case's name to "ok" or to what went wrong."""
import torch  # noqa: E402  (first: see above)

import importlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import explored_cases as xc  # noqa: E402
import np_explored as ne  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
SIZES = ((64, 40), (131, 67), (5, 9), (96, 200))
PAD = 8                                                        # sentinel words on each side of the rows
SENTINEL = 0xA5A5A5A5


def device_seen(ctx, ids, cls, words, off=0):
    """id (n, H, W) uint16 and cls (n, H, W) uint8 through dg_seen_lines_device: (n, words) uint32, after a check of the sentinel words
    around the rows.  off: bytes in front of both planes (2: the id plane is off the 16-byte boundary)."""
    n, H, W = ids.shape
    ti = torch.zeros(ids.nbytes + off, dtype=torch.uint8, device="cuda")
    ti[off:] = torch.from_numpy(np.ascontiguousarray(ids).reshape(-1).view(np.uint8)).cuda()
    tc = torch.zeros(cls.nbytes + off, dtype=torch.uint8, device="cuda")
    tc[off:] = torch.from_numpy(np.ascontiguousarray(cls).reshape(-1)).cuda()
    o = torch.from_numpy(np.full(n * words + 2 * PAD, SENTINEL, dtype=np.uint32).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    ctx.seen_lines_device(W, H, n, ti.data_ptr() + off, tc.data_ptr() + off, o.data_ptr() + 4 * PAD)
    got = o.cpu().numpy().view(np.uint32)
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + n * words:] == SENTINEL).all(), "words outside the rows were written"
    return got[PAD:PAD + n * words].reshape(n, words)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]:#x} model {want[tuple(bad[0])]:#x}"


def synthetic_case(ctx, ex, W, H):
    """The synthetic planes as one batch (rows must not mix), each alone, and three of them in another order."""
    names, ids, cls = xc.stacked(xc.synthetic_planes(ex, W, H))
    want = ex.seen(ids, cls)
    same(device_seen(ctx, ids, cls, ex.words), want, "batch")
    for k in range(len(names)):
        same(device_seen(ctx, ids[k:k + 1], cls[k:k + 1], ex.words), want[k:k + 1], names[k])
    pick = [len(names) - 1, 0, 2]
    same(device_seen(ctx, ids[pick], cls[pick], ex.words), want[pick], "n = 3")
    assert len({want[k].tobytes() for k in pick}) == 3                 # frames of different content
    t = ctx.seen_kernel_ms()
    assert t["lines_ms"] > 0.0 and t["accumulate_ms"] == 0.0, t


def unaligned_case(ctx, ex):
    """An id base 2 bytes off the 16-byte boundary (and a cls base with it) takes the any-alignment kernel whatever the size."""
    for W, H in ((64, 40), (96, 200)):
        names, ids, cls = xc.stacked(xc.synthetic_planes(ex, W, H))
        same(device_seen(ctx, ids, cls, ex.words, off=2), ex.seen(ids, cls), (W, H))


def many_segs_case(sw):
    """A grid map with more than 4 096 segs: the workgroup's seg bitset is more than 128 words."""
    wad = sw.build_synth_iwad(2002, grid=(18, 12), n_things=4)
    ex = ne.Explored(wad)
    assert len(ex.seg_line) > 4096
    scene = dg.Scene(wad, "e1m1")
    ctx = dg.Context(64, 40, max_batch=1, slots=1)
    ctx.upload_scene(scene)
    for W, H in ((131, 67), (96, 200)):
        names, ids, cls = xc.stacked(xc.synthetic_planes(ex, W, H))
        same(device_seen(ctx, ids, cls, ex.words), ex.seen(ids, cls), (W, H))
    ctx.close()
    scene.close()


def errors_case(ctx, wad):
    t = torch.zeros(65536, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    L = dg.lib()
    P = lambda v: None if v is None else dg._P(v)
    call = lambda c, W, H, n, i, k, s: L.dg_seen_lines_device(c, W, H, n, P(i), P(k), P(s))
    assert call(ctx._h, 8, 8, 1, p, p + 1024, p + 2048) == dg.DG_OK
    assert call(ctx._h, 8, 8, 1, p + 1, p + 1024, p + 2048) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert call(ctx._h, 8, 8, 1, p, p + 1024, p + 2050) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert call(ctx._h, 8, 8, 1, p + 2, p + 1027, p + 2052) == dg.DG_OK                      # cls sits anywhere
    for W, H, n in ((0, 8, 1), (8, 0, 1), (16385, 8, 1), (8, 8, -1)):
        assert call(ctx._h, W, H, n, p, p + 1024, p + 2048) == dg.DG_ERR_INVALID, (W, H, n)
    assert call(ctx._h, 8, 8, 0, p, p + 1024, p + 2048) == dg.DG_OK
    for k in range(3):
        ptrs = [p, p + 1024, p + 2048]
        ptrs[k] = None
        assert call(ctx._h, 8, 8, 1, *ptrs) == dg.DG_ERR_INVALID
    assert call(None, 8, 8, 1, p, p + 1024, p + 2048) == dg.DG_ERR_INVALID
    big = dg.Scene(xc.grow_map_lump(wad, "E1M1", 5, 12, 65537), "e1m1")                      # past the limit of label frames: 65 537 segs
    over = dg.Context(64, 40, max_batch=1, slots=1, front_end=dg.DG_FE_HOST)
    over.upload_scene(big)
    t[2048:2048 + 64] = 0xA5
    torch.cuda.synchronize()
    assert call(over._h, 8, 8, 1, p, p + 1024, p + 2048) == dg.DG_ERR_CAPACITY
    assert (t[2048:2048 + 64].cpu().numpy() == 0xA5).all()                                   # nothing was launched
    over.close()
    big.close()
    bare = dg.Context(64, 40, max_batch=1, slots=1)                                        # no scene uploaded
    assert call(bare._h, 8, 8, 1, p, p + 1024, p + 2048) == dg.DG_ERR_INVALID
    assert L.dg_ctx_seen_kernel_ms(bare._h, None, None) == dg.DG_ERR_INVALID                 # nothing launched yet
    bare.close()


def in_flight_case(scene, ex, path):
    """dg_seen_lines_device while label and bundle slots are in flight leaves their planes, counts and the fallback counters alone; the
    slot's own planes as the source give the slot's rows."""
    W, H, n = 320, 200, 16
    c = dg.Context(W, H, max_batch=3 * n, slots=2)
    c.upload_scene(scene)
    views = dg.make_views(path[0:960:60])
    c.submit_labels(0, views)
    c.submit_bundle(1, views, 7)
    want = (c.readback_labels(0, 0, n), c.readback(1, 0, n).copy(), c.readback_depth(1, 0, n), c.readback_labels(1, 0, n))
    t_want, fb_want = [c.timing(s) for s in (0, 1)], c.fallbacks()
    names, ids, cls = xc.stacked(xc.synthetic_planes(ex, 131, 67))
    c.submit_labels(0, views)
    got0 = device_seen(c, ids, cls, ex.words)                            # while slot 0's kernels run
    c.submit_bundle(1, views, 7)
    got1 = device_seen(c, ids[::-1], cls[::-1], ex.words)
    c.wait(0)
    c.wait(1)
    same(got0, ex.seen(ids, cls), "slot 0 in flight")
    same(got1, ex.seen(ids[::-1], cls[::-1]), "slot 1 in flight")
    counts = ("front_end", "n_frames", "n_spans", "covered_pixels")
    for slot in (0, 1):
        t = c.timing(slot)
        assert {k: t[k] for k in counts} == {k: t_want[slot][k] for k in counts}, (slot, t, t_want[slot])
    eq = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    assert eq(c.readback_labels(0, 0, n), want[0]) and np.array_equal(c.readback(1, 0, n), want[1])
    assert eq(c.readback_depth(1, 0, n), want[2]) and eq(c.readback_labels(1, 0, n), want[3])
    assert c.fallbacks() == fb_want
    lay = dg.bundle_layout(W, H, n, 7)
    for slot, id_at, cls_at, planes in ((0, 0, 2 * n * W * H, want[0]), (1, lay["id"], lay["cls"], want[3])):
        fb = c.framebuffer_ptr(slot)
        o = torch.zeros(n * ex.words * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.seen_lines_device(W, H, n, fb + id_at, fb + cls_at, o.data_ptr())
        rows = o.cpu().numpy().view(np.uint32).reshape(n, ex.words)
        same(rows, ex.seen(planes[0], planes[1]), f"slot {slot}'s planes")
        same(rows, c.slot_seen_lines(slot, 0, n, 1, want=("upto",))["upto"], f"slot {slot}: dg_slot_seen_lines")
    c.close()


def main(out_path):
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    wad = sw.build_synth_iwad(1993)
    scene, ex = dg.Scene(wad, "e1m1"), ne.Explored(wad)
    ctx = dg.Context(64, 40, max_batch=1, slots=1)
    ctx.upload_scene(scene)
    cases = {}
    for (W, H) in SIZES:
        cases[f"synthetic/{W}x{H}"] = lambda W=W, H=H: synthetic_case(ctx, ex, W, H)
    cases["unaligned"] = lambda: unaligned_case(ctx, ex)
    cases["many_segs"] = lambda: many_segs_case(sw)
    cases["errors"] = lambda: errors_case(ctx, wad)
    cases["in_flight"] = lambda: in_flight_case(scene, ex, path)
    results, stopped = {}, None
    for name, fn in cases.items():
        if stopped:                                                # after a HIP error nothing more goes to the GPU
            results[name] = f"not run: {stopped} ended in a HIP error"
            continue
        try:
            fn()
            results[name] = "ok"
        except Exception as e:                                     # an assertion or a DoomGpuError: the case's own result
            results[name] = traceback.format_exc()
            if isinstance(e, RuntimeError) and not isinstance(e, dg.DoomGpuError) or getattr(e, "code", 0) == dg.DG_ERR_HIP:
                stopped = name
    ctx.close()
    scene.close()
    with open(out_path, "w") as f:
        json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1])
