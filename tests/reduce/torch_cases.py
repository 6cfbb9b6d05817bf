"""torch_cases.py OUT.json — the cases of tests/test_reduce_gpu.py that hand torch tensors to dg_reduce_device, run in a process of
their own: a torch wheel that brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded, so that both resolve the
one runtime; in a pytest session the library is long loaded.  Every case is compared with the numpy restatement
(np_reduce) here; OUT.json maps a case's name to "ok" or to what went wrong."""
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
import np_reduce as npr  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
W0, H0, B0 = 320, 200, 16


def device_reduce(ctx, frames, fx, fy, fmt, src_off=0, dst_off=0):
    """frames (n, H, W, 3) uint8 through dg_reduce_device: the reduced bytes, after a check of the sentinel bytes around them."""
    n, H, W, _ = frames.shape
    src = torch.empty(frames.size + src_off, dtype=torch.uint8, device="cuda")
    src[src_off:] = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).cuda()
    nbytes = n * npr.reduced_size(W, H, fx, fy, fmt)[2]
    dst = torch.full((dst_off + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.reduce_device(src.data_ptr() + src_off, W, H, n, (fx, fy, fmt), dst.data_ptr() + dst_off)
    got = dst.cpu().numpy()
    assert (got[:dst_off] == 0xA5).all() and (got[dst_off + nbytes:] == 0xA5).all(), "bytes outside the destination were written"
    return got[dst_off:dst_off + nbytes]


def grid_case(ctx, frames, fx, fy):
    """1 and 3 frames of every content kind and 65 frames of all of them, both formats."""
    pick65 = np.arange(65) % len(frames)
    for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
        want = npr.reduce(frames, fx, fy, fmt)
        for k, kind in enumerate(npr.CONTENTS):
            for n in (1, 3):
                got = device_reduce(ctx, frames[3 * k:3 * k + n], fx, fy, fmt)
                assert np.array_equal(got, want[3 * k:3 * k + n].reshape(-1)), (kind, fmt, n)
        assert np.array_equal(device_reduce(ctx, frames[pick65], fx, fy, fmt), want[pick65].reshape(-1)), (fmt, 65)


def unaligned_case(ctx, frames):
    """A source one byte off a 16-byte boundary takes the any-width kernel whatever the width; the destination may sit anywhere too."""
    for fx, fy in npr.FACTORS:
        for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
            want = npr.reduce(frames, fx, fy, fmt).reshape(-1)
            assert np.array_equal(device_reduce(ctx, frames, fx, fy, fmt, src_off=1), want), (fx, fy, fmt, "source")
            assert np.array_equal(device_reduce(ctx, frames, fx, fy, fmt, src_off=16, dst_off=1), want), (fx, fy, fmt, "destination")


def framebuffer_case(ctx):
    """The slot's framebuffer as the source, a tensor as the destination: tensors without a host round trip."""
    full = ctx.readback(0, 0, B0)
    assert full.any()
    for fx, fy in ((4, 4), (5, 3)):
        for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
            want = npr.reduce(full, fx, fy, fmt)
            dst = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.reduce_device(ctx.framebuffer_ptr(0), W0, H0, B0, (fx, fy, fmt), dst.data_ptr())
            assert np.array_equal(dst.cpu().numpy(), want.reshape(-1)), (fx, fy, fmt)


def in_flight_case(scene, path):
    """dg_reduce_device while slots are in flight leaves their frames, their timing's counts and the fallback counters alone."""
    W, H, B = 640, 400, 64
    c = dg.Context(W, H, max_batch=B, slots=2, front_end=dg.DG_FE_DEVICE)      # (one front end: the timing's counts are comparable)
    c.upload_scene(scene)
    views = dg.make_views(path[0:B])
    want = c.render(views).copy()
    t_want, fb_want = c.timing(0), c.fallbacks()
    frames = npr.content("random", 5, 131, 67)
    c.submit(0, views)
    got = device_reduce(c, frames, 3, 3, dg.DG_REDUCE_RGB24)               # while slot 0's kernels run
    c.submit(1, views)
    got_gray = device_reduce(c, frames, 7, 3, dg.DG_REDUCE_GRAY8)
    assert c.reduce_kernel_ms() > 0.0
    c.wait(0)
    c.wait(1)
    assert np.array_equal(got, npr.reduce(frames, 3, 3).reshape(-1)) and np.array_equal(got_gray, npr.reduce(frames, 7, 3, npr.GRAY8).reshape(-1))
    counts = ("front_end", "n_frames", "n_spans", "covered_pixels")
    for slot in (0, 1):
        t = c.timing(slot)
        assert {k: t[k] for k in counts} == {k: t_want[k] for k in counts}, (slot, t, t_want)
        assert t["raster_ms"] > 0.0 and t["total_ms"] >= t["raster_ms"], t
        assert np.array_equal(c.readback(slot, 0, B), want), slot
    assert c.fallbacks() == fb_want
    c.close()


def main(out_path):
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(W0, H0, max_batch=B0, slots=2)
    ctx.upload_scene(scene)
    ctx.submit(0, dg.make_views(path[0:960:60]))
    ctx.wait(0)
    frames = {(W, H): np.concatenate([npr.content(kind, 3, W, H) for kind in npr.CONTENTS]) for W, H in npr.SIZES}
    cases = {}
    for (W, H) in npr.SIZES:
        for (fx, fy) in npr.FACTORS:
            cases[f"grid/{W}x{H}/{fx}x{fy}"] = lambda W=W, H=H, fx=fx, fy=fy: grid_case(ctx, frames[(W, H)], fx, fy)
    for (W, H) in ((64, 40), (131, 67), (320, 200)):
        cases[f"unaligned/{W}x{H}"] = lambda W=W, H=H: unaligned_case(ctx, frames[(W, H)][:3])
    cases["framebuffer"] = lambda: framebuffer_case(ctx)
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
