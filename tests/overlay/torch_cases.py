"""torch_cases.py OUT.json — the cases of tests/test_overlay_gpu.py that hand a torch buffer to dg_overlay_device.
They run in a process of their own: a torch wheel that brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded
(INTEGRATION.md), and in a pytest session the library is long loaded.  Every frame of every case is compared in full with dg_overlay_host
and with the numpy painter (np_overlay, through overlay_cases.expected), and sentinel bytes in front of and behind the frames are checked.
OUT.json maps a case's name to "ok", to "out of memory: ..." or to what went wrong.  After a HIP error nothing more is sent to the GPU."""
import torch  # noqa: E402  (first: see above)

import gc
import importlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_cases as oc  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
PAD = 4099                                                     # sentinel bytes in front of and behind the frames (odd: the frames sit off every alignment)
TWO32 = 1 << 32
EDGE = 64 * 1024


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first (frame, y, x) = {bad[0].tolist()}: gpu {got[tuple(bad[0])].tolist()} want {want[tuple(bad[0])].tolist()}")


def device_case(ctx, scene, W, H, name):
    """One case list through dg_overlay_device on a torch buffer: against the host twin, against the painter, and the sentinels."""
    items = oc.hud_frames(W, H) if name == "hud" else oc.cases(W, H)[name]
    base = oc.base_frames(W, H, len(items))
    t = torch.full((base.size + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    t[PAD:PAD + base.size] = torch.from_numpy(base.reshape(-1)).cuda()
    torch.cuda.synchronize()
    ctx.overlay_device(t.data_ptr() + PAD, W, H, items)
    got = t.cpu().numpy()
    assert (got[:PAD] == 0xA5).all() and (got[PAD + base.size:] == 0xA5).all(), f"{name}: bytes outside the frames were written"
    got = got[PAD:PAD + base.size].reshape(base.shape)
    same(got, dg.overlay_host(scene, base.copy(), items), (name, "host twin"))
    same(got, oc.expected(W, H, name), (name, "painter"))
    assert ctx.overlay_kernel_ms() > 0.0 or not any(items)


def past_4_gib_case(ctx, scene):
    """1280 x 800 frames in an uninitialised buffer just over 4 GiB, the screen on frame 0 and on the last frame only: those two frames in
    full, and 64 KiB on either side of the 4 GiB mark untouched."""
    W, H = 1280, 800
    fb = 3 * W * H
    n = TWO32 // fb + 2
    assert (n - 1) * fb > TWO32 + EDGE and (n - 2) * fb < TWO32 - EDGE + fb
    t = torch.empty((n * fb,), dtype=torch.uint8, device="cuda")
    base = oc.base_frames(W, H, 3)
    t[:fb] = torch.from_numpy(base[0].reshape(-1)).cuda()
    t[(n - 1) * fb:] = torch.from_numpy(base[2].reshape(-1)).cuda()
    t[TWO32 - EDGE:TWO32 + EDGE] = 0x5A
    torch.cuda.synchronize()
    frames = oc.hud_frames(W, H)
    ctx.overlay_device(t.data_ptr(), W, H, [frames[0]] + [[]] * (n - 2) + [frames[2]])
    want = oc.expected(W, H, "hud")
    same(t[:fb].cpu().numpy().reshape(1, H, W, 3), want[0:1], "frame 0")
    same(t[(n - 1) * fb:].cpu().numpy().reshape(1, H, W, 3), want[2:3], "the last frame")
    assert bool((t[TWO32 - EDGE:TWO32 + EDGE] == 0x5A).all()), "bytes around the 4 GiB mark were written"
    assert (want[0] != base[0]).any() and (want[2] != base[2]).any()


def main(out_path):
    scene = oc.load(dg)
    ctx = dg.Context(64, 40, max_batch=1, slots=1)                            # (the frames' size is the call's, not the ctx's)
    ctx.upload_scene(scene)
    cases = {}
    for (W, H) in oc.SIZES:
        for name in oc.cases(W, H):
            cases[f"cases/{W}x{H}/{name}"] = lambda W=W, H=H, name=name: device_case(ctx, scene, W, H, name)
    cases["hud/1280x800"] = lambda: device_case(ctx, scene, 1280, 800, "hud")
    cases["big/past 4 GiB"] = lambda: past_4_gib_case(ctx, scene)
    results, stopped = {}, None
    for name, fn in cases.items():
        if stopped:                                                # after a HIP error nothing more goes to the GPU
            results[name] = f"not run: {stopped} ended in a HIP error"
            continue
        try:
            fn()
            results[name] = "ok"
        except torch.cuda.OutOfMemoryError as e:                   # the case's test skips with this reason
            results[name] = f"out of memory: {e}"
        except Exception as e:                                     # an assertion or a DoomGpuError: the case's own result
            results[name] = traceback.format_exc()
            if isinstance(e, RuntimeError) and not isinstance(e, dg.DoomGpuError) or getattr(e, "code", 0) == dg.DG_ERR_HIP:
                stopped = name
        print(f"{name}  {results[name].splitlines()[-1][:200]}", flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    ctx.close()
    scene.close()
    with open(out_path, "w") as f:
        json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1])
