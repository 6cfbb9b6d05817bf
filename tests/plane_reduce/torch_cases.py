"""torch_cases.py OUT.json — the cases of tests/test_plane_reduce_gpu.py that hand torch tensors to dg_reduce_planes_device, run in a
process of their own: a torch wheel that brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded, so that both
resolve the one runtime; in a pytest session the library is long loaded.  Every case is compared with the numpy
restatement (np_plane_reduce) here; OUT.json maps a case's name to "ok" or to what went wrong."""
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
import np_plane_reduce as npp  # noqa: E402
import np_reduce as npr  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
RULES = (npp.POINT, npp.NEAREST)
PAD = 32                                                       # sentinel elements on each side of every destination
SENTINEL = {"distance": 0x5A5A, "kind": 0xA5, "id": 0xA5A5, "cls": 0xA5}


def device_reduce(ctx, planes, fx, fy, rule, src_off=0):
    """planes {name: (n, H, W)} through dg_reduce_planes_device: {name: (n, oH, oW)}, after a check of the sentinel elements around every
    destination.  src_off: elements in front of every source plane (1: the distance plane is off a 16-byte boundary)."""
    n, H, W = next(iter(planes.values())).shape
    oW, oH = npp.reduced_size(W, H, fx, fy)
    src, dst, keep = {}, {}, {}
    for k, a in planes.items():                                 # (every tensor is a byte tensor: the planes' own dtypes stay on the numpy side)
        off = src_off * a.itemsize
        t = torch.zeros(a.nbytes + off, dtype=torch.uint8, device="cuda")
        t[off:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()
        o = torch.from_numpy(np.full(n * oW * oH + 2 * PAD, SENTINEL[k], dtype=npp.DTYPES[k]).view(np.uint8)).cuda()
        keep[k] = (t, o)
        src[k] = t.data_ptr() + off
        dst[k] = o.data_ptr() + PAD * a.itemsize
    torch.cuda.synchronize()
    ctx.reduce_planes_device(W, H, n, (fx, fy, rule), src, dst)
    out = {}
    for k, (t, o) in keep.items():
        got = o.cpu().numpy().view(npp.DTYPES[k])
        s = np.array(SENTINEL[k], dtype=np.uint16).astype(npp.DTYPES[k])
        assert (got[:PAD] == s).all() and (got[PAD + n * oW * oH:] == s).all(), f"elements outside the {k} destination were written"
        out[k] = got[PAD:PAD + n * oW * oH].reshape(n, oH, oW)
    return out


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {len(bad)} {k} entries differ, first at {bad[0].tolist()}: gpu {got[k][tuple(bad[0])]} model {want[k][tuple(bad[0])]}"


def contents(W, H, fx, fy):
    """3 frames of every distance content with the tracer planes: (12, H, W) each."""
    planes = npp.tracer_planes(3 * len(npp.CONTENTS), W, H)
    planes["distance"] = np.concatenate([npp.distance_content(kind, 3, W, H, fx, fy) for kind in npp.CONTENTS])
    return planes


def grid_case(ctx, W, H, fx, fy):
    """1 and 3 frames of every content kind and 65 frames of all of them, both rules; pairs left out."""
    planes = contents(W, H, fx, fy)
    pick65 = np.arange(65) % (3 * len(npp.CONTENTS))
    for rule in RULES:
        want = npp.reduce(rule, fx, fy, **planes)
        for k, kind in enumerate(npp.CONTENTS):
            for n in (1, 3):
                got = device_reduce(ctx, {name: a[3 * k:3 * k + n] for name, a in planes.items()}, fx, fy, rule)
                same(got, {name: a[3 * k:3 * k + n] for name, a in want.items()}, (kind, rule, n))
        same(device_reduce(ctx, {name: a[pick65] for name, a in planes.items()}, fx, fy, rule), {name: a[pick65] for name, a in want.items()}, (rule, 65))
        for names in (("distance",), ("distance", "id"), ("distance", "kind", "cls")) + ((("id", "cls"), ("kind",)) if rule == npp.POINT else ()):
            same(device_reduce(ctx, {name: planes[name][:3] for name in names}, fx, fy, rule), {name: want[name][:3] for name in names}, (rule, names))


def unaligned_case(ctx, W, H):
    """Sources one element off a 16-byte boundary take the any-width kernel whatever the width."""
    for fx, fy in npr.FACTORS:
        planes = {k: a[:6] for k, a in contents(W, H, fx, fy).items()}
        for rule in RULES:
            same(device_reduce(ctx, planes, fx, fy, rule, src_off=1), npp.reduce(rule, fx, fy, **planes), (fx, fy, rule))


def errors_case(ctx):
    """What dg_reduce_planes_device refuses before it launches: odd addresses of 16-bit planes, NEAREST without the distance plane, a
    source without its destination; and what it accepts without launching."""
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    L = dg.lib()
    P = lambda v: None if v is None else dg._P(v)
    def call(desc, src, dst, n=1):
        d = dg.DgPlaneReduceDesc(*desc, 0)
        return L.dg_reduce_planes_device(ctx._h, 8, 8, n, d, *[P(v) for v in src], *[P(v) for v in dst])
    assert call((2, 2, 1), (p, None, None, None), (p + 1024, None, None, None)) == dg.DG_OK
    assert ctx.plane_reduce_kernel_ms() >= 0.0
    for src, dst in (((p + 1, None, None, None), (p + 1024, None, None, None)), ((p, None, None, None), (p + 1025, None, None, None)),
                     ((p, None, p + 257, None), (p + 1024, None, p + 2048, None)), ((p, None, p + 256, None), (p + 1024, None, p + 2049, None))):
        assert call((2, 2, 1), src, dst) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert call((2, 2, 1), (None, p, None, None), (None, p + 1024, None, None)) == dg.DG_ERR_INVALID
    assert call((2, 2, 0), (None, p + 1, None, p + 3), (None, p + 1025, None, p + 2049)) == dg.DG_OK       # 8-bit planes sit anywhere
    assert call((2, 2, 0), (p, None, None, None), (None, None, None, None)) == dg.DG_ERR_INVALID
    assert call((2, 2, 0), (None, None, None, None), (None, None, p, None)) == dg.DG_ERR_INVALID
    assert call((2, 2, 0), (None,) * 4, (None,) * 4) == dg.DG_OK
    assert call((2, 2, 1), (p, None, None, None), (p + 1024, None, None, None), n=0) == dg.DG_OK
    assert call((2, 2, 1), (p, None, None, None), (p + 1024, None, None, None), n=-1) == dg.DG_ERR_INVALID
    for desc in ((0, 2, 0), (2, 17, 0), (2, 2, 2)):
        assert call(desc, (p, None, None, None), (p + 1024, None, None, None)) == dg.DG_ERR_INVALID
    assert L.dg_reduce_planes_device(ctx._h, 8, 8, 1, dg.DgPlaneReduceDesc(2, 2, 0, 1), P(p), None, None, None, P(p + 1024), None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduce_planes_device(ctx._h, 8, 8, 1, None, P(p), None, None, None, P(p + 1024), None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduce_planes_device(ctx._h, 0, 8, 1, dg.DgPlaneReduceDesc(2, 2, 0, 0), P(p), None, None, None, P(p + 1024), None, None, None) == dg.DG_ERR_INVALID


def in_flight_case(scene, path):
    """dg_reduce_planes_device while bundle slots are in flight leaves their planes, their timing's counts and the fallback counters alone."""
    W, H, n = 320, 200, 16
    c = dg.Context(W, H, max_batch=3 * n, slots=2)
    c.upload_scene(scene)
    views = dg.make_views(path[0:960:60])
    c.submit_bundle(0, views, 7)
    want = (c.readback(0, 0, n).copy(), c.readback_depth(0, 0, n), c.readback_labels(0, 0, n))
    t_want, fb_want = c.timing(0), c.fallbacks()
    planes = {k: a[:5] for k, a in contents(131, 67, 3, 3).items()}
    c.submit_bundle(0, views, 7)
    got = device_reduce(c, planes, 3, 3, npp.NEAREST)                  # while slot 0's kernels run
    c.submit_bundle(1, views, 7)
    got_pt = device_reduce(c, planes, 7, 3, npp.POINT)
    assert c.plane_reduce_kernel_ms() > 0.0
    c.wait(0)
    c.wait(1)
    same(got, npp.reduce(npp.NEAREST, 3, 3, **planes), "nearest")
    same(got_pt, npp.reduce(npp.POINT, 7, 3, **planes), "point")
    counts = ("front_end", "n_frames", "n_spans", "covered_pixels")
    for slot in (0, 1):
        t = c.timing(slot)
        assert {k: t[k] for k in counts} == {k: t_want[k] for k in counts}, (slot, t, t_want)
        assert t["total_ms"] > 0.0, t
        assert np.array_equal(c.readback(slot, 0, n), want[0]), slot
        assert all(np.array_equal(a, b) for a, b in zip(c.readback_depth(slot, 0, n), want[1])), slot
        assert all(np.array_equal(a, b) for a, b in zip(c.readback_labels(slot, 0, n), want[2])), slot
    assert c.fallbacks() == fb_want
    # the slot's own planes as the source, tensors as the destination: against the reduced readback's rule on the same planes
    lay = dg.bundle_layout(W, H, n, 7)
    fb = c.framebuffer_ptr(0)
    full = dict(zip(npp.NAMES, want[1] + want[2][:2]))
    oW, oH = npp.reduced_size(W, H, 4, 4)
    outs = {k: torch.zeros(n * oW * oH * full[k].itemsize, dtype=torch.uint8, device="cuda") for k in npp.NAMES}
    torch.cuda.synchronize()
    c.reduce_planes_device(W, H, n, (4, 4, npp.NEAREST), {k: fb + lay[k] for k in npp.NAMES}, {k: outs[k].data_ptr() for k in npp.NAMES})
    same({k: outs[k].cpu().numpy().view(npp.DTYPES[k]).reshape(n, oH, oW) for k in npp.NAMES}, npp.reduce(npp.NEAREST, 4, 4, **full), "slot planes into tensors")
    c.close()


def main(out_path):
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(64, 40, max_batch=1, slots=1)
    cases = {}
    for (W, H) in npr.SIZES:
        for (fx, fy) in npr.FACTORS:
            cases[f"grid/{W}x{H}/{fx}x{fy}"] = lambda W=W, H=H, fx=fx, fy=fy: grid_case(ctx, W, H, fx, fy)
    cases["unaligned/64x40"] = lambda: unaligned_case(ctx, 64, 40)
    cases["errors"] = lambda: errors_case(ctx)
    cases["in_flight"] = lambda: in_flight_case(scene, path)
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
