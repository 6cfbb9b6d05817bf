"""torch_cases.py OUT.json [TIMES.json] — the cases of tests/test_extents_gpu.py, which hand torch tensors to dg_reduce_device,
dg_reduce_planes_device, dg_observe_device and dg_seen_lines_device at the extents no other test reaches: rows of
more than one run, more frames than one launch holds, and buffers past 2^32 bytes.  They run in a process of their own: a torch wheel that
brings its own HIP runtime has to be imported BEFORE libdoomgpu.so is loaded, so that both resolve the one runtime; in
a pytest session the library is long loaded.  Every case is compared with the numpy restatements (np_reduce, np_plane_reduce,
np_observe, np_explored) as bit patterns, every destination pre-filled with sentinels and with sentinel elements in front of and behind
it.  OUT.json maps a case's name to "ok", to "out of memory: ..." or to what went wrong; TIMES.json to its seconds.  After a HIP error
nothing more is sent to the GPU."""
import torch  # noqa: E402  (first: see above)

import gc
import importlib
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extent_cases as ec  # noqa: E402
import np_explored as ne  # noqa: E402
import np_observe as npo  # noqa: E402
import np_plane_reduce as npp  # noqa: E402
import np_reduce as npr  # noqa: E402

dg = importlib.import_module("doom-rust-renderer_amd")
PAD = 32                                                       # sentinel elements in front of and behind every destination
SENTINEL = {"distance": 0x5A5A, "kind": 0xA5, "id": 0xA5A5, "cls": 0xA5}
RULES = (npp.POINT, npp.NEAREST)
BIG = 16                                                       # box size of the sources past 2^32: the destination stays small


def upload(a, off=0):
    """A numpy array as device bytes `off` bytes behind an allocation's start: (the tensor to keep, the device address)."""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.zeros(raw.size + off, dtype=torch.uint8, device="cuda")
    t[off:] = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + off


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: gpu {int(got[tuple(bad[0])]):#x} model {int(want[tuple(bad[0])]):#x}")


def padded(want, fill):
    """The flat expected elements with PAD sentinel elements on each side."""
    pad = np.full(PAD, fill, dtype=want.dtype)
    return np.concatenate([pad, want.reshape(-1), pad])


def run_reduce(ctx, ptr, W, H, n, fx, fy, fmt, want, what):
    """dg_reduce_device into a sentinel buffer: the whole buffer against the model's bytes with sentinels around."""
    dst = torch.full((want.size + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.reduce_device(ptr, W, H, n, (fx, fy, fmt), dst.data_ptr() + PAD)
    same(dst.cpu().numpy(), padded(want, 0xA5), what)


def run_planes(ctx, ptrs, W, H, n, fx, fy, rule, want, what):
    """dg_reduce_planes_device of the planes in `want` into sentinel buffers, each whole buffer against the model's."""
    keep = {k: torch.from_numpy(np.full(v.size + 2 * PAD, SENTINEL[k], dtype=v.dtype).view(np.uint8)).cuda() for k, v in want.items()}
    torch.cuda.synchronize()
    ctx.reduce_planes_device(W, H, n, (fx, fy, rule), {k: ptrs[k] for k in want}, {k: t.data_ptr() + PAD * want[k].itemsize for k, t in keep.items()})
    for k, t in keep.items():
        same(t.cpu().numpy().view(want[k].dtype), padded(want[k], np.array(SENTINEL[k], dtype=np.uint16).astype(want[k].dtype)), (what, k))


_addresses = {}


def placed(bits, name):
    """np_observe.placed with the addresses of a (layout, shape) worked out once: (the expected buffer, base, strides)."""
    key = (name, bits.shape)
    if key not in _addresses:
        total, base, strides = npo.layout(name, *bits.shape)
        at = npo.addresses(bits.shape, base, strides).reshape(-1)
        assert np.unique(at).size == at.size and at.max(initial=0) < max(total, 1)
        _addresses[key] = (total, base, strides, at)
    total, base, strides, at = _addresses[key]
    buf = np.full(total * bits.dtype.itemsize, 0xA5, dtype=np.uint8).view(bits.dtype)
    buf[at] = bits.reshape(-1)
    return buf, base, strides


def desc(source, rule, fx, fy, dtype, m):
    scale, bias, lo, hi = m
    return dg.DgObsDesc(fx, fy, source, rule, dtype, lo, hi, float(scale), float(bias), 0)


def run_observe(ctx, ptr, W, H, n, d, name, want_bits, what):
    """dg_observe_device of n frames into layout `name` of a sentinel buffer with PAD elements around it; the whole buffer against the
    model's bits placed the same way."""
    want, base, strides = placed(want_bits, name)
    eb = want.itemsize
    pad = npo.sentinel(PAD, d.dtype)
    t = torch.full(((want.size + 2 * PAD) * eb,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.observe_device(ptr, W, H, n, d, t.data_ptr() + (PAD + base) * eb, strides)
    same(t.cpu().numpy().view(want.dtype), np.concatenate([pad, want, pad]), what)


# ---- B: past the first run -----------------------------------------------------------------------------------------------------------------

def reduce_shape_case(ctx, shape):
    """RGB24 and GRAY8 of one frame of every content at every box size of the table."""
    W, H0, un = shape
    uploads = {}
    for fx, fy in npr.FACTORS:
        H = ec.height_of(H0, fy)
        if H not in uploads:
            frames = ec.colour_frames(W, H)
            uploads[H] = (frames,) + upload(frames, 1 if un else 0)
        frames, keep, ptr = uploads[H]
        for fmt in (npr.RGB24, npr.GRAY8):
            run_reduce(ctx, ptr, W, H, len(frames), fx, fy, fmt, npr.reduce(frames, fx, fy, fmt), (fx, fy, fmt))


def planes_shape_case(ctx, shape):
    """NEAREST and POINT, all four planes: every distance content under per-frame tracer planes, at every box size of the table."""
    W, H0, un = shape
    for fx, fy in npr.FACTORS:
        H = ec.height_of(H0, fy)
        planes = ec.plane_sources(W, H, fx, fy)
        ups = {k: upload(a, (2 if un else 0)) for k, a in planes.items()}
        for rule in RULES:
            run_planes(ctx, {k: p for k, (t, p) in ups.items()}, W, H, len(planes["id"]), fx, fy, rule, npp.reduce(rule, fx, fy, **planes), (fx, fy, rule))


def observe_shape_case(ctx, shape, source, rule):
    """Every dtype x layout at every box size of the table; the maps and the frame counts (2, 3, 5) take turns."""
    W, H0, un = shape
    k, counts = 0, (2, 3, 5)
    for fx, fy in npr.FACTORS:
        H = ec.height_of(H0, fy)
        src = npo.sources(source, max(counts), W, H, fx, fy)
        v = npo.values(source, rule, fx, fy, src)
        keep, ptr = upload(src, (2 if source == npo.DISTANCE else 1) if un else 0)
        for dtype in npo.DTYPES:
            maps = list(npo.maps_for(dtype).values())
            for name in npo.LAYOUTS:
                m, n = maps[k % len(maps)], counts[k % 3]
                run_observe(ctx, ptr, W, H, n, desc(source, rule, fx, fy, dtype, m), name, npo.convert(v[:n], dtype, m[2], m[3], m[0], m[1]),
                            (fx, fy, dtype, name, n))
                k += 1


# ---- C: past the first launch ----------------------------------------------------------------------------------------------------------------
_chunk_sources = {}


def chunk_source(kind, W, H):
    """The most frames any case takes, random per frame, uploaded once per (kind, shape): (numpy, tensor, address)."""
    key = (kind, W, H)
    if key not in _chunk_sources:
        n = max(ec.FRAME_COUNTS)
        a = ec.random_frames(n, H, W, seed=11) if kind == "colour" else ec.random_distance(n, H, W, seed=12)
        assert (a[:n - ec.CHUNK] != a[ec.CHUNK:]).reshape(n - ec.CHUNK, -1).any(axis=1).all()    # no frame equals the one a launch before it
        _chunk_sources[key] = (a,) + upload(a)
    return _chunk_sources[key]


def reduce_chunks_case(ctx, W, H, n):
    frames, keep, ptr = chunk_source("colour", W, H)
    for fmt in (npr.RGB24, npr.GRAY8):
        run_reduce(ctx, ptr, W, H, n, 2, 2, fmt, npr.reduce(frames[:n], 2, 2, fmt), fmt)
        assert ctx.reduce_kernel_ms() > 0.0


def planes_chunks_case(ctx, W, H, n):
    dist, keep, ptr = chunk_source("distance", W, H)
    rng = np.random.default_rng([13, W, H])
    ids = rng.integers(0, 65536, size=dist.shape, dtype=np.uint16)
    planes = {"distance": dist[:n], "kind": (ids[:n] >> 3 & 3).astype(np.uint8), "id": ids[:n], "cls": (ids[:n] & 7).astype(np.uint8)}
    ups = {k: upload(a) for k, a in planes.items() if k != "distance"}
    ptrs = dict({k: p for k, (t, p) in ups.items()}, distance=ptr)
    for rule in RULES:
        run_planes(ctx, ptrs, W, H, n, 2, 2, rule, npp.reduce(rule, 2, 2, **planes), rule)
        assert ctx.plane_reduce_kernel_ms() > 0.0


# kind -> the (dtype, layout) pairs its cases past one launch write: every dtype and layout under both item maps and all five kernels
CHUNK_OUTPUTS = {(npo.RGB, 0): ((npo.F32, "nchw"), (npo.F16, "nhwc")), (npo.GRAY, 0): ((npo.U8, "slice"), (npo.BF16, "nchw")),
                 (npo.DISTANCE, npp.POINT): ((npo.F32, "nhwc"), (npo.U8, "nchw")), (npo.DISTANCE, npp.NEAREST): ((npo.F16, "slice"), (npo.BF16, "nchw"))}


def observe_chunks_case(ctx, W, H, n, colour):
    src, keep, ptr = chunk_source("colour" if colour else "distance", W, H)
    for (source, rule), outputs in CHUNK_OUTPUTS.items():
        if (source != npo.DISTANCE) != colour:
            continue
        v = npo.values(source, rule, 2, 2, src[:n])
        for dtype, name in outputs:
            m = npo.U8_MAPS["u8_full"] if dtype == npo.U8 else npo.MAPS["unit"] if colour else npo.MAPS["far"]
            run_observe(ctx, ptr, W, H, n, desc(source, rule, 2, 2, dtype, m), name, npo.convert(v, dtype, m[2], m[3], m[0], m[1]), (source, rule, dtype, name))
            assert ctx.observe_kernel_ms() > 0.0


def run_seen(ctx, id_ptr, cls_ptr, W, H, n, want, what):
    o = torch.from_numpy(np.full(want.size + 2 * PAD, 0xA5A5A5A5, dtype=np.uint32).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    ctx.seen_lines_device(W, H, n, id_ptr, cls_ptr, o.data_ptr() + 4 * PAD)
    same(o.cpu().numpy().view(np.uint32), padded(want, 0xA5A5A5A5), what)


def seen_chunks_case(ctx, ex, W, H, n):
    key = ("seen", W, H)
    if key not in _chunk_sources:
        ids, cls = ec.random_labels(max(ec.FRAME_COUNTS), H, W, len(ex.seg_line), seed=14)
        _chunk_sources[key] = (ids, cls, ec.seen_rows(ex, ids, cls), upload(ids), upload(cls))
    ids, cls, rows, (k1, id_ptr), (k2, cls_ptr) = _chunk_sources[key]
    at = sorted({0, 1, ec.CHUNK - 1, ec.CHUNK, ec.CHUNK + 1, n - 1})
    same(rows[at], ex.seen(ids[at], cls[at]), "the fast model against np_explored")
    k = max(ec.FRAME_COUNTS) - ec.CHUNK
    assert (rows[:k] != rows[ec.CHUNK:]).any(axis=1).mean() > 0.5            # a launch that read the frames of the one before could not pass
    run_seen(ctx, id_ptr, cls_ptr, W, H, n, rows[:n], n)
    t = ctx.seen_kernel_ms()
    assert t["lines_ms"] > 0.0, t


# ---- D: past 2^32 --------------------------------------------------------------------------------------------------------------------------

def tiled(base, n):
    """base (K, ...) numpy -> a (n, bytes) uint8 tensor on the GPU: frame i is base[i % K]."""
    K = base.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(base).reshape(K, -1).view(np.uint8)).cuda()
    return b.repeat(n // K, 1)


def big_inputs(entry, base):
    """n and the host-side condition of a source past 2^32: the bytes a wrapped 32-bit offset of the first frame behind the boundary would
    reach differ from that frame's own (whole frame; the base frames alone decide)."""
    flat = np.ascontiguousarray(base).reshape(ec.K_BASE, -1).view(np.uint8)
    fb = flat.shape[1]
    n = ec.big_frames(fb)
    f, wrapped = ec.first_frame_behind(fb)
    assert n * fb > ec.TWO32 and f + 1 < n and ec.wrapped_bytes_differ(flat, f, wrapped, length=fb), entry
    return n


def check_tiled(dst, nbytes, want, what):
    """dst: PAD sentinel bytes, n frames, PAD sentinel bytes; want (K, ...) numpy.  On the GPU."""
    n_pad = (dst.numel() - nbytes) // 2
    K = want.shape[0]
    w = torch.from_numpy(np.ascontiguousarray(want).reshape(K, -1).view(np.uint8)).cuda()
    body = dst[n_pad:n_pad + nbytes].view(-1, K, w.shape[1])
    assert bool((dst[:n_pad] == 0xA5).all()) and bool((dst[n_pad + nbytes:] == 0xA5).all()), f"{what}: bytes outside the destination were written"
    if not torch.equal(body, w.unsqueeze(0).expand_as(body)):
        bad = (body != w.unsqueeze(0)).flatten(1).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{what}: groups of {K} frames that differ from the model: {bad.numel()}, first {int(bad[0])}")


def big_reduce_source_case(ctx):
    W, H, _ = ec.BIG_SOURCES["reduce"]
    base = ec.random_frames(ec.K_BASE, H, W, seed=21)
    n = big_inputs("reduce", base)
    src = tiled(base, n)
    for fmt in (npr.RGB24, npr.GRAY8):
        want = npr.reduce(base, BIG, BIG, fmt)
        assert len({w.tobytes() for w in want}) == ec.K_BASE
        nbytes = n * want[0].size
        dst = torch.full((nbytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.reduce_device(src.data_ptr(), W, H, n, (BIG, BIG, fmt), dst.data_ptr() + PAD)
        check_tiled(dst, nbytes, want, fmt)


def big_planes_source_case(ctx, rule):
    """NEAREST: distance and cls; POINT: id and kind (two planes of 2 and 1 bytes per pixel: 6 GiB)."""
    W, H, _ = ec.BIG_SOURCES["planes"]
    rng = np.random.default_rng([22, rule])
    wide, narrow = ("distance", "cls") if rule == npp.NEAREST else ("id", "kind")
    planes = {wide: rng.integers(0, 65536, size=(ec.K_BASE, H, W), dtype=np.uint16).view(npp.DTYPES[wide]),
              narrow: rng.integers(0, 256, size=(ec.K_BASE, H, W), dtype=np.uint8)}
    n = big_inputs("planes", planes[wide])
    src = {k: tiled(a, n) for k, a in planes.items()}
    want = npp.reduce(rule, BIG, BIG, **planes)
    dst = {k: torch.full((n * v[0].nbytes + 2 * PAD * v.itemsize,), 0xA5, dtype=torch.uint8, device="cuda") for k, v in want.items()}
    torch.cuda.synchronize()
    ctx.reduce_planes_device(W, H, n, (BIG, BIG, rule), {k: t.data_ptr() for k, t in src.items()}, {k: t.data_ptr() + PAD * want[k].itemsize for k, t in dst.items()})
    for k in want:
        assert len({w.tobytes() for w in want[k]}) == ec.K_BASE
        check_tiled(dst[k], n * want[k][0].nbytes, want[k], (rule, k))


def big_observe_source_case(ctx, source, rule, dtype):
    W, H, _ = ec.BIG_SOURCES["observe_distance" if source == npo.DISTANCE else "observe_rgb"]
    base = ec.random_distance(ec.K_BASE, H, W, seed=23) if source == npo.DISTANCE else ec.random_frames(ec.K_BASE, H, W, seed=23)
    n = big_inputs("observe", base)
    src = tiled(base, n)
    m = npo.U8_MAPS["u8_full"] if dtype == npo.U8 else npo.MAPS["identity"] if source == npo.DISTANCE else npo.MAPS["unit"]
    want = npo.observe(base, source, rule, BIG, BIG, dtype, m[2], m[3], m[0], m[1])              # (K, C, oH, oW) bit patterns
    assert len({w.tobytes() for w in want}) == ec.K_BASE
    eb, per = want.itemsize, want[0].size
    dst = torch.full(((n * per + 2 * PAD) * eb,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    C, oH, oW = want.shape[1:]
    ctx.observe_device(src.data_ptr(), W, H, n, desc(source, rule, BIG, BIG, dtype, m), dst.data_ptr() + PAD * eb, (per, oH * oW, oW, 1))
    check_tiled(dst, n * per * eb, want, (source, rule, dtype))


def big_seen_source_case(ctx, ex):
    """Three base frames of floor with 27 wall pixels each, other segs per frame, from the first band to the last."""
    W, H, _ = ec.BIG_SOURCES["seen"]
    px, S = W * H, len(ex.seg_line)
    ids, cls = np.zeros((ec.K_BASE, px), np.uint16), np.full((ec.K_BASE, px), 3, np.uint8)
    for k in range(ec.K_BASE):
        at = np.arange(k, px, 20011)
        at[-1] = px - 1 - k
        ids[k, at] = (np.arange(len(at)) * 7 + 31 * k) % S
        cls[k, at] = 1
    ids, cls = ids.reshape(ec.K_BASE, H, W), cls.reshape(ec.K_BASE, H, W)
    n = big_inputs("seen", ids)
    want = ex.seen(ids, cls)
    assert len({w.tobytes() for w in want}) == ec.K_BASE and want.any(axis=1).all()
    ti, tc = tiled(ids, n), tiled(cls, n)
    nbytes = n * ex.words * 4
    dst = torch.full((nbytes + 8 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.seen_lines_device(W, H, n, ti.data_ptr(), tc.data_ptr(), dst.data_ptr() + 4 * PAD)
    check_tiled(dst, nbytes, want, "seen")


def big_identity_case(ctx, entry):
    """A destination past 2^32 bytes under 1 x 1 boxes, where the output is the source: dg_reduce_device (RGB24), dg_reduce_planes_device
    NEAREST (distance) and POINT (id).  Source and destination are 4 GiB each: a destination that large has a source no smaller."""
    W, H, _ = ec.BIG_SOURCES["reduce" if entry == "reduce" else "planes"]
    base = ec.random_frames(ec.K_BASE, H, W, seed=24) if entry == "reduce" else ec.random_distance(ec.K_BASE, H, W, seed=24)
    n = big_inputs(entry, base)
    src = tiled(base, n)
    eb = 1 if entry == "reduce" else 2
    dst = torch.full((src.numel() + 2 * PAD * eb,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    at = dst.data_ptr() + PAD * eb
    if entry == "reduce":
        ctx.reduce_device(src.data_ptr(), W, H, n, (1, 1, npr.RGB24), at)
    elif entry == "nearest":
        ctx.reduce_planes_device(W, H, n, (1, 1, npp.NEAREST), {"distance": src.data_ptr()}, {"distance": at})
    else:
        ctx.reduce_planes_device(W, H, n, (1, 1, npp.POINT), {"id": src.data_ptr()}, {"id": at})
    assert bool((dst[:PAD * eb] == 0xA5).all()) and bool((dst[PAD * eb + src.numel():] == 0xA5).all()), "bytes outside the destination were written"
    body = dst[PAD * eb:PAD * eb + src.numel()].view(src.shape)
    if not torch.equal(body, src):
        bad = (body != src).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{entry}: {bad.numel()} frames differ from their source, first {int(bad[0])}")


def big_stride_case(ctx, dtype, st0):
    """dg_observe_device with a frame stride of st0 elements: two 131 x 67 frames under 3 x 3, every kind in turn.  The frames and PAD
    elements around each are checked, not the 4 GiB between them."""
    W, H, fx, fy, n = 131, 67, 3, 3, 2
    oW, oH = npp.reduced_size(W, H, fx, fy)
    eb = np.dtype(npo.BITS[dtype]).itemsize
    assert (st0 * eb > ec.TWO32) and (st0 > ec.TWO32) == (dtype == npo.U8)
    extent = 3 * oH * oW
    t = torch.full(((PAD + st0 + extent + PAD) * eb,), 0xA5, dtype=torch.uint8, device="cuda")
    m = npo.U8_MAPS["u8_full"] if dtype == npo.U8 else npo.MAPS["unit"]
    for source, rule in npo.KINDS:
        src = npo.sources(source, n, W, H, fx, fy)
        src[1] = src[1][::-1, ::-1]                                            # (the two frames differ whatever the content)
        want = npo.observe(src, source, rule, fx, fy, dtype, m[2], m[3], m[0], m[1])
        assert want[0].tobytes() != want[1].tobytes()
        keep, ptr = upload(src)
        torch.cuda.synchronize()
        ctx.observe_device(ptr, W, H, n, desc(source, rule, fx, fy, dtype, m), t.data_ptr() + PAD * eb, (st0, oH * oW, oW, 1))
        for f in range(n):
            lo = f * st0 * eb
            got = t[lo:lo + (2 * PAD + extent) * eb].cpu().numpy().view(want.dtype)
            same(got, np.concatenate([npo.sentinel(PAD, dtype), want[f].reshape(-1), npo.sentinel(extent - want[f].size + PAD, dtype)]), (source, rule, f))
            t[lo:lo + (2 * PAD + extent) * eb] = 0xA5


def main(out_path, times_path=None):
    sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")
    wad = sw.build_synth_iwad(1993)
    scene, ex = dg.Scene(wad, "e1m1"), ne.Explored(wad)
    ctx = dg.Context(64, 40, max_batch=1, slots=1)
    ctx.upload_scene(scene)
    cases = {}
    for shape in ec.SHAPES:
        sid = ec.shape_id(shape)
        cases[f"runs/reduce/{sid}"] = lambda shape=shape: reduce_shape_case(ctx, shape)
        cases[f"runs/planes/{sid}"] = lambda shape=shape: planes_shape_case(ctx, shape)
        for (source, rule) in npo.KINDS:
            cases[f"runs/observe/{sid}/source{source}rule{rule}"] = lambda shape=shape, source=source, rule=rule: observe_shape_case(ctx, shape, source, rule)
    for n in ec.FRAME_COUNTS:
        for form in (0, 1):
            tag = f"{n}/{'any' if form else '16'}"
            size = lambda entry: ec.CHUNK_SHAPES[entry][form]
            cases[f"chunks/reduce/{tag}"] = lambda n=n, s=size("reduce"): reduce_chunks_case(ctx, *s, n)
            cases[f"chunks/planes/{tag}"] = lambda n=n, s=size("planes"): planes_chunks_case(ctx, *s, n)
            cases[f"chunks/observe_rgb/{tag}"] = lambda n=n, s=size("observe_rgb"): observe_chunks_case(ctx, *s, n, True)
            cases[f"chunks/observe_distance/{tag}"] = lambda n=n, s=size("observe_distance"): observe_chunks_case(ctx, *s, n, False)
            cases[f"chunks/seen/{tag}"] = lambda n=n, s=size("seen"): seen_chunks_case(ctx, ex, *s, n)
    cases["big/source/reduce"] = lambda: big_reduce_source_case(ctx)
    cases["big/source/planes_nearest"] = lambda: big_planes_source_case(ctx, npp.NEAREST)
    cases["big/source/planes_point"] = lambda: big_planes_source_case(ctx, npp.POINT)
    cases["big/source/observe_rgb"] = lambda: big_observe_source_case(ctx, npo.RGB, 0, npo.F32)
    cases["big/source/observe_nearest"] = lambda: big_observe_source_case(ctx, npo.DISTANCE, npp.NEAREST, npo.F16)
    cases["big/source/observe_point"] = lambda: big_observe_source_case(ctx, npo.DISTANCE, npp.POINT, npo.U8)
    cases["big/source/seen"] = lambda: big_seen_source_case(ctx, ex)
    cases["big/destination/reduce"] = lambda: big_identity_case(ctx, "reduce")
    cases["big/destination/planes_nearest"] = lambda: big_identity_case(ctx, "nearest")
    cases["big/destination/planes_point"] = lambda: big_identity_case(ctx, "point")
    cases["big/destination/observe_u8_stride"] = lambda: big_stride_case(ctx, npo.U8, ec.TWO32 + 4099)
    cases["big/destination/observe_f32_bytes"] = lambda: big_stride_case(ctx, npo.F32, (1 << 30) + 1027)
    only = os.environ.get("EXTENT_CASES")                                # a prefix: run these cases alone (measurements)
    results, times, stopped = {}, {}, None
    for name, fn in cases.items():
        if only and not name.startswith(only):
            continue
        if stopped:                                                # after a HIP error nothing more goes to the GPU
            results[name] = f"not run: {stopped} ended in a HIP error"
            continue
        if name.startswith("big/"):                                # one such case alive at a time
            _chunk_sources.clear()
            gc.collect()
            torch.cuda.empty_cache()
        t0 = time.perf_counter()
        try:
            fn()
            results[name] = "ok"
        except torch.cuda.OutOfMemoryError as e:                   # the case's test skips with this reason
            results[name] = f"out of memory: {e}"
        except Exception as e:                                     # an assertion or a DoomGpuError: the case's own result
            results[name] = traceback.format_exc()
            if isinstance(e, RuntimeError) and not isinstance(e, dg.DoomGpuError) or getattr(e, "code", 0) == dg.DG_ERR_HIP:
                stopped = name
        times[name] = round(time.perf_counter() - t0, 3)
        print(f"{times[name]:8.3f} s  {name}  {results[name].splitlines()[-1][:200]}", flush=True)
        gc.collect()
        if name.startswith("big/"):
            torch.cuda.empty_cache()
    ctx.close()
    scene.close()
    with open(out_path, "w") as f:
        json.dump(results, f)
    if times_path:
        with open(times_path, "w") as f:
            json.dump(times, f)


if __name__ == "__main__":
    main(*sys.argv[1:3])
