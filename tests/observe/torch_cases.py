"""torch_cases.py OUT.json — the cases of tests/test_observe_gpu.py, which hand torch tensors to dg_observe_device, run in a process of
their own: a torch wheel that brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded, so that both resolve the one
runtime; in a pytest session the library is long loaded.  Every case is compared with the numpy restatement
(np_observe) here, as bit patterns; OUT.json maps a case's name to "ok" or to what went wrong.  After a HIP error nothing more is sent
to the GPU."""
import torch  # noqa: E402  (first: see above)

import ctypes
import importlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_observe as npo  # noqa: E402
import np_plane_reduce as npp  # noqa: E402
import np_reduce as npr  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
PAD = 32                                                       # sentinel elements in front of and behind every destination buffer
BASE_FRAMES = 5                                                # the frames a case's sources are made of (every content kind is in)
TORCH = {npo.U8: torch.uint8, npo.F16: torch.float16, npo.BF16: torch.bfloat16, npo.F32: torch.float32}
SIGNED = {1: torch.uint8, 2: torch.int16, 4: torch.int32}     # the integer view of a tensor's elements


def desc(source, rule, fx, fy, dtype, m):
    scale, bias, lo, hi = m
    return dg.DgObsDesc(fx, fy, source, rule, dtype, lo, hi, float(scale), float(bias), 0)


def upload(a, off=0):
    """A numpy array as device bytes `off` bytes behind an allocation's start: (the tensor to keep, the device address)."""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.zeros(raw.size + off, dtype=torch.uint8, device="cuda")
    t[off:] = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + off


def bits_of(t):
    """A tensor's elements as numpy bit patterns, in the tensor's own shape."""
    eb = t.element_size()
    return t.contiguous().view(SIGNED[eb]).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[eb])


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: gpu {got[tuple(bad[0])]:#x} model {want[tuple(bad[0])]:#x}"


def device_check(ctx, src_ptr, W, H, n, d, name, want_bits, what):
    """dg_observe_device of n frames into layout `name` of a sentinel buffer with PAD elements around it; the whole buffer against the
    model's bits placed the same way."""
    want, base, strides = npo.placed(want_bits, name)
    eb = want.itemsize
    pad = npo.sentinel(PAD, d.dtype)
    t = torch.from_numpy(np.concatenate([pad, npo.sentinel(want.size, d.dtype), pad]).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    ctx.observe_device(src_ptr, W, H, n, d, t.data_ptr() + (PAD + base) * eb, strides)
    same(t.cpu().numpy().view(want.dtype), np.concatenate([pad, want, pad]), what)


def grid_case(ctx, W, H, fx, fy):
    """(RGB, F32, NCHW) under the 1/255 map: 1, 3 and 65 frames."""
    src = npo.sources(npo.RGB, BASE_FRAMES, W, H, fx, fy)
    counts = (1, 3, 65) if W * H <= 131 * 67 else (1, 3)
    pick = np.arange(max(counts)) % BASE_FRAMES
    v = npo.values(npo.RGB, 0, fx, fy, src)[pick]
    keep, ptr = upload(src[pick])
    m = npo.MAPS["unit"]
    for n in counts:
        device_check(ctx, ptr, W, H, n, desc(npo.RGB, 0, fx, fy, npo.F32, m), "nchw", npo.convert(v[:n], npo.F32, m[2], m[3], m[0], m[1]), n)


def combos_case(ctx, W, H, source, rule, off=0):
    """Every dtype x layout at four box sizes; the frame counts (1, 3, 65) and the maps take turns.  off: bytes the source sits behind a
    16-byte boundary (the any-width kernels at every width)."""
    k = 0
    counts = (1, 3, 65) if W * H <= 131 * 67 else (1, 3, 2)
    pick = np.arange(max(counts)) % BASE_FRAMES
    for fx, fy in ((1, 1), (3, 3), (7, 3), (16, 16)):
        src = npo.sources(source, BASE_FRAMES, W, H, fx, fy)
        v = npo.values(source, rule, fx, fy, src)[pick]
        keep, ptr = upload(src[pick], off)
        for dtype in npo.DTYPES:
            maps = list(npo.maps_for(dtype).values())
            for name in npo.LAYOUTS:
                m = maps[k % len(maps)]
                n = counts[k % 3]
                device_check(ctx, ptr, W, H, n, desc(source, rule, fx, fy, dtype, m), name, npo.convert(v[:n], dtype, m[2], m[3], m[0], m[1]),
                             (fx, fy, dtype, name, n, m))
                k += 1


def maps_case(ctx, source, rule):
    """Every map on every dtype, at 131x67 under 3x3, 4 frames."""
    W, H, fx, fy = 131, 67, 3, 3
    src = npo.sources(source, 4, W, H, fx, fy)
    if source == npo.DISTANCE:
        src[0, :2, :6] = np.array([[0, 1, -1, 2048, 2049, -32768], [32767, 2047, 77, 76, 78, 3]], dtype=np.int16)
    v = npo.values(source, rule, fx, fy, src)
    keep, ptr = upload(src)
    for dtype in npo.DTYPES:
        for name, m in npo.maps_for(dtype).items():
            device_check(ctx, ptr, W, H, 4, desc(source, rule, fx, fy, dtype, m), "nchw", npo.convert(v, dtype, m[2], m[3], m[0], m[1]), (dtype, name))


def sweep_case(ctx):
    """Every int16 once, through observe_into and tensors of the four dtypes (U8 under the clamp it needs)."""
    src = npo.sweep_frame()
    keep, ptr = upload(src)
    for dtype in npo.DTYPES:
        lo, hi = (0, 255) if dtype == npo.U8 else npo.FULL
        t = torch.zeros((1, 1, 256, 256), dtype=TORCH[dtype], device="cuda")
        torch.cuda.synchronize()
        ctx.observe_into(ptr, 256, 256, 1, desc(npo.DISTANCE, npp.POINT, 1, 1, dtype, (1, 0, lo, hi)), t)
        same(bits_of(t).reshape(-1), npo.convert(src.reshape(-1), dtype, lo, hi, 1, 0), dtype)
    for bad in (torch.zeros((1, 1, 256, 255), dtype=torch.float16, device="cuda"), torch.zeros((1, 1, 256, 256), dtype=torch.float32, device="cuda")):
        try:
            ctx.observe_into(ptr, 256, 256, 1, desc(npo.DISTANCE, npp.POINT, 1, 1, npo.F16, npo.MAPS["identity"]), bad)
        except ValueError:
            continue
        raise AssertionError("observe_into took a tensor of another shape or dtype")


def composed_case(ctx):
    """RGB into channels 0..2 and distance into channel 3 of one float16 tensor by two calls; gray into slot t % 4 of a stack over 6 steps.
    Both against the model, untouched elements included."""
    W, H, fx, fy, n = 131, 67, 3, 3, 3
    oW, oH = npp.reduced_size(W, H, fx, fy)
    rgb, dist = npo.sources(npo.RGB, n, W, H, fx, fy), npo.sources(npo.DISTANCE, n, W, H, fx, fy)
    k1, p_rgb = upload(rgb)
    k2, p_dist = upload(dist)
    unit, far = npo.MAPS["unit"], npo.MAPS["far"]
    t = torch.full((n, 4, oH, oW), 7.0, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    ctx.observe_into(p_rgb, W, H, n, desc(npo.RGB, 0, fx, fy, npo.F16, unit), t[:, :3])
    after_rgb = bits_of(t)
    ctx.observe_into(p_dist, W, H, n, desc(npo.DISTANCE, npp.NEAREST, fx, fy, npo.F16, far), t[:, 3:])
    want = np.full((n, 4, oH, oW), np.float16(7.0).view(np.uint16), dtype=np.uint16)
    want[:, :3] = npo.observe(rgb, npo.RGB, 0, fx, fy, npo.F16, unit[2], unit[3], unit[0], unit[1])
    same(after_rgb, want, "RGB-D after the colour call")                    # channel 3 still holds 7.0
    want[:, 3:] = npo.observe(dist, npo.DISTANCE, npp.NEAREST, fx, fy, npo.F16, far[2], far[3], far[0], far[1])
    same(bits_of(t), want, "RGB-D")
    # a frame stack: at step s every environment's newest gray frame goes to slot s % 4 (channel-sliced, one call per step)
    envs, steps = 2, 6
    frames = npo.sources(npo.GRAY, envs * steps, W, H, fx, fy).reshape(steps, envs, H, W, 3)
    stack = torch.zeros((envs, 4, oH, oW), dtype=torch.float32, device="cuda")
    want = np.zeros((envs, 4, oH, oW), dtype=np.uint32)
    signed = npo.MAPS["signed"]
    for s in range(steps):
        keep, ptr = upload(frames[s])
        torch.cuda.synchronize()
        ctx.observe_into(ptr, W, H, envs, desc(npo.GRAY, 0, fx, fy, npo.F32, signed), stack[:, s % 4:s % 4 + 1])
        want[:, s % 4:s % 4 + 1] = npo.observe(frames[s], npo.GRAY, 0, fx, fy, npo.F32, signed[2], signed[3], signed[0], signed[1])
        same(bits_of(stack), want, ("stack", s))


def errors_case(ctx):
    """What dg_observe_device refuses before it launches, and what it accepts without launching."""
    L = dg.lib()
    fresh = dg.Context(64, 40, max_batch=1, slots=1)
    try:
        fresh.observe_kernel_ms()
        raise AssertionError("observe_kernel_ms before any call")
    except dg.DoomGpuError as e:
        assert e.code == dg.DG_ERR_INVALID
    fresh.close()
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    st = (48, 16, 4, 1)
    def call(d, src, dst, strides=st, n=1, W=8, H=8, c=ctx._h):
        return L.dg_observe_device(c, None if src is None else dg._P(src), W, H, n, None if d is None else d, None if dst is None else dg._P(dst),
                                   None if strides is None else (ctypes.c_int64 * 4)(*strides))
    ok = dg.DgObsDesc(2, 2, dg.DG_OBS_RGB, 0, dg.DG_OBS_F32, -32768, 32767, 1.0, 0.0, 0)
    dist = dg.DgObsDesc(2, 2, dg.DG_OBS_DISTANCE, dg.DG_PLANE_NEAREST, dg.DG_OBS_F16, -32768, 32767, 1.0, 0.0, 0)
    assert call(ok, p, p + 4096) == dg.DG_OK and ctx.observe_kernel_ms() >= 0.0
    assert call(ok, p, p + 4096, n=0) == dg.DG_OK
    assert call(ok, p + 1, p + 4096) == dg.DG_OK                                                  # a colour source sits anywhere
    assert call(dist, p + 2, p + 4096 + 2, (16, 16, 4, 1)) == dg.DG_OK
    t[4096:] = 0x5A
    torch.cuda.synchronize()
    for args in ((None, p, p + 4096), (ok, None, p + 4096), (ok, p, None), (ok, p, p + 4096, None)):
        assert call(*args) == dg.DG_ERR_INVALID
    assert call(ok, p, p + 4096, c=None) == dg.DG_ERR_INVALID
    assert call(ok, p, p + 4096, n=-1) == dg.DG_ERR_INVALID
    for (w, h) in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        assert call(ok, p, p + 4096, W=w, H=h) == dg.DG_ERR_INVALID
    assert call(dist, p + 1, p + 4096, (16, 16, 4, 1)) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert call(dist, p, p + 4097, (16, 16, 4, 1)) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert call(ok, p, p + 4098) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    for strides in ((48, 16, 4, 0), (48, 16, -4, 1), (48, 16, 3, 1), (16, 16, 4, 1), (48, 16, 4, 4)):
        assert call(ok, p, p + 4096, strides, n=2) == dg.DG_ERR_INVALID and b"stride" in L.dg_last_error(), strides
    D = dg.DgObsDesc
    for d in (D(0, 2, 0, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 17, 0, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 3, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 0, 1, 3, 0, 255, 1.0, 0.0, 0),
              D(2, 2, 2, 2, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 0, 0, 4, 0, 255, 1.0, 0.0, 0), D(2, 2, 0, 0, 3, 0, 255, 1.0, 0.0, 1), D(2, 2, 0, 0, 3, 5, 4, 1.0, 0.0, 0),
              D(2, 2, 0, 0, 3, 0, 40000, 1.0, 0.0, 0), D(2, 2, 0, 0, 3, 0, 255, float("inf"), 0.0, 0), D(2, 2, 0, 0, 3, 0, 255, 1.0, float("nan"), 0),
              D(2, 2, 0, 0, 0, 0, 255, 0.5, 0.0, 0), D(2, 2, 0, 0, 0, 0, 256, 1.0, 0.0, 0)):
        assert call(d, p, p + 4096) == dg.DG_ERR_INVALID
    assert bool((t[4096:] == 0x5A).all())                                                        # a refused call writes nothing


def slot_case(scene, path):
    """The slot's own frames and distance plane as sources (framebuffer_ptr, bundle_layout), against the model over readback /
    readback_depth of the same slot; then observations while two slots are in flight leave the slots alone."""
    W, H, n = 320, 200, 16
    what = dg.DG_BUNDLE_COLOUR | dg.DG_BUNDLE_DEPTH
    c = dg.Context(W, H, max_batch=3 * n, slots=2)
    c.upload_scene(scene)
    views = dg.make_views(path[0:960:60])
    c.submit_bundle(0, views, what)
    frames = c.readback(0, 0, n).copy()
    distance, kind = c.readback_depth(0, 0, n)
    assert frames.any() and (distance != 32767).any()
    t_want, fb_want = c.timing(0), c.fallbacks()
    lay = dg.bundle_layout(W, H, n, what)
    fb = c.framebuffer_ptr(0)
    unit, far = npo.MAPS["unit"], npo.MAPS["far"]
    cases = [(npo.RGB, 0, 4, 4, npo.F16, unit, fb + lay["colour"], frames), (npo.GRAY, 0, 2, 2, npo.U8, npo.U8_MAPS["u8_full"], fb + lay["colour"], frames),
             (npo.RGB, 0, 1, 1, npo.F32, unit, fb + lay["colour"], frames), (npo.DISTANCE, npp.NEAREST, 4, 4, npo.F16, far, fb + lay["distance"], distance),
             (npo.DISTANCE, npp.POINT, 5, 3, npo.BF16, far, fb + lay["distance"], distance)]
    def run_all(tag):
        for (source, rule, fx, fy, dtype, m, ptr, src) in cases:
            oW, oH = npp.reduced_size(W, H, fx, fy)
            t = torch.zeros((n, npo.channels(source), oH, oW), dtype=TORCH[dtype], device="cuda")
            torch.cuda.synchronize()
            c.observe_into(ptr, W, H, n, desc(source, rule, fx, fy, dtype, m), t)
            same(bits_of(t), npo.observe(src, source, rule, fx, fy, dtype, m[2], m[3], m[0], m[1]), (tag, source, rule, fx, fy, dtype))
    run_all("slot sources")
    # in flight: sources in tensors of their own, while slot 0's and slot 1's kernels run
    k1, p_rgb = upload(frames[:5])
    k2, p_dist = upload(distance[:5])
    outs = []
    c.submit_bundle(0, views, what)
    for (source, rule, fx, fy, dtype, m, ptr, src) in ((npo.RGB, 0, 3, 3, npo.F16, unit, p_rgb, frames[:5]), (npo.DISTANCE, npp.NEAREST, 7, 3, npo.F32, far, p_dist, distance[:5])):
        oW, oH = npp.reduced_size(W, H, fx, fy)
        t = torch.zeros((5, npo.channels(source), oH, oW), dtype=TORCH[dtype], device="cuda")
        torch.cuda.synchronize()
        c.observe_into(ptr, W, H, 5, desc(source, rule, fx, fy, dtype, m), t)
        outs.append((t, npo.observe(src, source, rule, fx, fy, dtype, m[2], m[3], m[0], m[1])))
        c.submit_bundle(1, views, what)
    assert c.observe_kernel_ms() > 0.0
    c.wait(0)
    c.wait(1)
    for t, want in outs:
        same(bits_of(t), want, "in flight")
    counts = ("front_end", "n_frames", "n_spans", "covered_pixels")
    for slot in (0, 1):
        t = c.timing(slot)
        assert {k: t[k] for k in counts} == {k: t_want[k] for k in counts}, (slot, t, t_want)
        assert t["total_ms"] > 0.0, t
        assert np.array_equal(c.readback(slot, 0, n), frames), slot
        assert all(np.array_equal(a, b) for a, b in zip(c.readback_depth(slot, 0, n), (distance, kind))), slot
    assert c.fallbacks() == fb_want
    c.close()


def main(out_path):
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
    scene = dg.Scene(sw.build_synth_iwad(1993), "e1m1")
    ctx = dg.Context(64, 40, max_batch=1, slots=1)
    cases = {"errors": lambda: errors_case(ctx)}
    for (W, H) in npr.SIZES:
        for (fx, fy) in npr.FACTORS:
            cases[f"grid/{W}x{H}/{fx}x{fy}"] = lambda W=W, H=H, fx=fx, fy=fy: grid_case(ctx, W, H, fx, fy)
        for (source, rule) in npo.KINDS:
            cases[f"combos/{W}x{H}/source{source}rule{rule}"] = lambda W=W, H=H, source=source, rule=rule: combos_case(ctx, W, H, source, rule)
    for (source, rule) in npo.KINDS:
        cases[f"unaligned/source{source}rule{rule}"] = lambda source=source, rule=rule: combos_case(ctx, 64, 40, source, rule, off=2 if source == npo.DISTANCE else 1)
        cases[f"maps/source{source}rule{rule}"] = lambda source=source, rule=rule: maps_case(ctx, source, rule)
    cases["sweep"] = lambda: sweep_case(ctx)
    cases["composed"] = lambda: composed_case(ctx)
    cases["slot"] = lambda: slot_case(scene, path)
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
