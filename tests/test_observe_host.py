"""CPU tier of the observation tensors: dg_observe_host and dg_observed_size against the numpy restatement
(np_observe), bit pattern for bit pattern — every comparison is on unsigned views, so signed zeros and infinities are pinned.

  grid          np_reduce.SIZES x np_reduce.FACTORS for (RGB, F32, NCHW); every source/rule x dtype x layout (contiguous NCHW,
                channels-last, a channel slice of a padded buffer with a long frame stride) at four sizes x four box sizes, the whole
                buffer compared, so the sentinel bytes outside the addressed elements too
  maps          every map of np_observe.MAPS (identity, 1/255, 2/255 - 1, negation, float32 / float16 subnormals, float16 / float32
                infinity, a far clamp, lo == hi) on every source and wide dtype
  sweep         one 256x256 distance frame with every int16, through F16, BF16 and F32
  narrowing     the host's two narrowing functions over > 10^6 structured float32 patterns against .astype(np.float16) and the model's
                bfloat16, the latter cross-checked against torch on the CPU in a child process
  errors        every error return of the contract, the stride rule's accepts and refusals, the exports, observe_into
  stand-alone   tests/observe/observe_host_main.cpp under AddressSanitizer + UBSan, as a program
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import np_observe as npo
import np_plane_reduce as npp
import np_reduce as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
P = ctypes.c_void_p
SIZES = [(64, 40), (131, 67), (5, 9), (1, 1)]
FACTORS = [(1, 1), (3, 3), (7, 3), (16, 16)]
N = 3


def desc(dg, source, rule, fx, fy, dtype, m):
    scale, bias, lo, hi = m
    return dg.DgObsDesc(fx, fy, source, rule, dtype, lo, hi, float(scale), float(bias), 0)


def host_into(dg, src, d, name):
    """dg_observe_host into layout `name` of a sentinel buffer: the whole buffer as bit patterns."""
    n, H, W = src.shape[:3]
    C, oH, oW, eb = dg.observed_size(W, H, d)
    total, base, strides = npo.layout(name, n, C, oH, oW)
    buf = npo.sentinel(total, d.dtype)
    assert buf.itemsize == eb
    rc = dg.lib().dg_observe_host(src.ctypes.data_as(P), W, H, n, ctypes.byref(d), P(buf.ctypes.data + base * eb), (ctypes.c_int64 * 4)(*strides))
    assert rc == dg.DG_OK, dg.lib().dg_last_error()
    return buf


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[0]}: host {got[bad[0]]:#x} model {want[bad[0]]:#x}"


def check(dg, src, source, rule, fx, fy, dtype, m, name, v=None):
    v = npo.values(source, rule, fx, fy, src) if v is None else v
    want, _, _ = npo.placed(npo.convert(v, dtype, m[2], m[3], m[0], m[1]), name)
    same(host_into(dg, src, desc(dg, source, rule, fx, fy, dtype, m), name), want, (source, rule, fx, fy, dtype, m, name))


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_rgb_f32_nchw_over_the_reduce_grid(dg, size, factor):
    (W, H), (fx, fy) = size, factor
    src = npo.sources(npo.RGB, len(npr.CONTENTS), W, H, fx, fy)
    check(dg, src, npo.RGB, 0, fx, fy, npo.F32, npo.MAPS["unit"], "nchw")
    got = dg.observe_host(src, desc(dg, npo.RGB, 0, fx, fy, npo.F32, npo.MAPS["unit"]))           # the binding returns the same, as float32
    assert got.dtype == np.float32 and got.shape == (len(src), 3) + npr.reduced_size(W, H, fx, fy)[1::-1]
    same(got.view(np.uint32).reshape(-1), npo.observe(src, npo.RGB, 0, fx, fy, npo.F32, *npo.FULL, *npo.MAPS["unit"][:2]).reshape(-1), "binding")


@pytest.mark.parametrize("kind", npo.KINDS, ids=lambda k: f"source{k[0]}rule{k[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_source_dtype_and_layout(dg, kind, size):
    (source, rule), (W, H) = kind, size
    k = 0
    for fx, fy in FACTORS:
        n = max(N, len(npp.CONTENTS if source == npo.DISTANCE else npr.CONTENTS))       # every content kind is in
        src = npo.sources(source, n, W, H, fx, fy)
        v = npo.values(source, rule, fx, fy, src)
        for dtype in npo.DTYPES:
            maps = list(npo.maps_for(dtype).values())
            for name in npo.LAYOUTS:
                check(dg, src, source, rule, fx, fy, dtype, maps[k % len(maps)], name, v)     # (the maps take turns; all of them: below)
                k += 1


@pytest.mark.parametrize("kind", npo.KINDS, ids=lambda k: f"source{k[0]}rule{k[1]}")
def test_every_map(dg, kind):
    source, rule = kind
    W, H, fx, fy = 131, 67, 3, 3
    src = npo.sources(source, 4, W, H, fx, fy)
    if source == npo.DISTANCE:
        src[0, :2, :6] = np.array([[0, 1, -1, 2048, 2049, -32768], [32767, 2047, 77, 76, 78, 3]], dtype=np.int16)
    v = npo.values(source, rule, fx, fy, src)
    for dtype in npo.DTYPES:
        for name, m in npo.maps_for(dtype).items():
            check(dg, src, source, rule, fx, fy, dtype, m, "nchw", v)
    # the maps do what their names say, in the model the host was just held to
    z = npo.convert(np.array([0]), npo.F32, *npo.FULL, *npo.MAPS["negate"][:2])
    assert z[0] == 0x00000000                                                              # 0 * -1 + 0 = +0, not -0
    assert npo.convert(np.array([1]), npo.F32, *npo.FULL, *npo.MAPS["f32_subnormal"][:2])[0] == 1 << 9        # 2^-140: a subnormal, kept
    assert npo.convert(np.array([1]), npo.F16, *npo.FULL, *npo.MAPS["f16_subnormal"][:2])[0] == 1 << 4        # 2^-20 = 16 x 2^-24
    assert npo.convert(np.array([255, -255]), npo.F16, *npo.FULL, *npo.MAPS["f16_infinity"][:2]).tolist() == [0x7C00, 0xFC00]
    assert npo.convert(np.array([32767, -32768]), npo.F32, *npo.FULL, *npo.MAPS["f32_infinity"][:2]).tolist() == [0x7F800000, 0xFF800000]
    assert npo.convert(np.array([5000]), npo.F32, *npo.MAPS["far"][2:], *npo.MAPS["far"][:2])[0] == 0x3F800000     # min(d, far) / far = 1


def test_the_sweep_of_every_int16(dg):
    src = npo.sweep_frame()
    assert np.unique(src).size == 65536
    for dtype in (npo.F16, npo.BF16, npo.F32):
        got = dg.observe_host(src, desc(dg, npo.DISTANCE, npp.POINT, 1, 1, dtype, npo.MAPS["identity"]))
        bits = got.view(npo.BITS[dtype]).reshape(-1)
        same(bits, npo.convert(src.reshape(-1), dtype, *npo.FULL, 1, 0), dtype)
    # what the sweep holds: float16 overflow is impossible (|v| <= 32768 < 65520) but ties are not
    f16 = npo.convert(src.reshape(-1), npo.F16, *npo.FULL, 1, 0).view(np.float16).astype(np.int64)
    assert f16[32768 + 2049] == 2048 and f16[32768 + 2051] == 2052 and f16[0] == -32768          # ties to even, both ways


@pytest.fixture(scope="module")
def narrowed(tmp_path_factory):
    """The host's narrowing functions over npo.structured_f32_patterns(): (patterns, float16 bits, bfloat16 bits)."""
    d = tmp_path_factory.mktemp("observe_narrow")
    exe, fin, fout = d / "narrow_main", d / "in.u32", d / "out.u16"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "observe", "narrow_main.cpp")])
    pat = npo.structured_f32_patterns()
    pat.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, dtype=np.uint16)
    assert out.size == 2 * pat.size
    return pat, out[:pat.size], out[pat.size:]


def test_host_narrowing_over_structured_patterns(narrowed):
    pat, f16, bf16 = narrowed
    assert pat.size >= 10 ** 6 and np.unique(pat >> 23).size == 512          # every exponent, both signs
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want16 = pat.view(np.float32).astype(np.float16).view(np.uint16)
    same(f16, want16, "binary16")
    same(bf16, npo.bf16_bits(pat), "bfloat16")
    finite = (pat & 0x7FFFFFFF) < 0x7F800000
    assert (f16[finite] & 0x7FFF).max() == 0x7C00 and (bf16[finite] & 0x7FFF).max() == 0x7F80      # overflow reaches infinity, never a NaN
    assert ((f16[finite] & 0x7C00) == 0).any() and (f16[finite] & 0x7FFF).min() == 0                # subnormals and zeros are in


def test_bf16_model_equals_torch_on_the_cpu(narrowed, tmp_path):
    """The model's bfloat16 narrowing against torch's, in a child process that imports torch first."""
    pat, _, bf16 = narrowed
    fin, fout = tmp_path / "in.u32", tmp_path / "out.u16"
    pat.tofile(fin)
    code = ("import torch, numpy as np, sys\n"
            "u = np.fromfile(sys.argv[1], dtype=np.uint32)\n"
            "t = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16)\n"
            "t.view(torch.int16).numpy().view(np.uint16).tofile(sys.argv[2])\n")
    r = subprocess.run([sys.executable, "-c", code, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.fromfile(fout, dtype=np.uint16)
    nan = (pat & 0x7FFFFFFF) > 0x7F800000
    same(got[~nan], bf16[~nan], "torch bfloat16")
    assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x7F) != 0).all()               # a NaN stays a NaN on both sides


def test_observed_size(dg):
    for (W, H) in npr.SIZES:
        for (fx, fy) in npr.FACTORS:
            oW, oH = npp.reduced_size(W, H, fx, fy)
            for (source, rule) in npo.KINDS:
                for dtype in npo.DTYPES:
                    d = desc(dg, source, rule, fx, fy, dtype, list(npo.maps_for(dtype).values())[0])
                    assert dg.observed_size(W, H, d) == (npo.channels(source), oH, oW, np.dtype(npo.BITS[dtype]).itemsize)
    d = desc(dg, npo.RGB, 0, 2, 2, npo.F16, npo.MAPS["unit"])
    assert dg.lib().dg_observed_size(8, 8, ctypes.byref(d), None, None, None, None) == dg.DG_OK      # every output is optional
    assert dg.lib().dg_observed_size(16384, 16384, ctypes.byref(d), None, None, None, None) == dg.DG_OK


def _call(dg, d, src, dst, strides, W=8, H=8, n=1, fn="dg_observe_host"):
    st = None if strides is None else (ctypes.c_int64 * 4)(*strides)
    return getattr(dg.lib(), fn)(src, W, H, n, None if d is None else ctypes.byref(d), dst, st)


def test_contract_errors(dg):
    L = dg.lib()
    inf, nan = float("inf"), float("nan")
    src = np.zeros(8 * 8 * 3 + 8, np.uint8)
    dst = np.full(4096, 0x5A, np.uint8)
    sp, dp = P(src.ctypes.data), P(dst.ctypes.data)
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0
    ok = dg.DgObsDesc(2, 2, dg.DG_OBS_RGB, 0, dg.DG_OBS_F32, -32768, 32767, 1.0, 0.0, 0)
    st = (48, 16, 4, 1)
    assert _call(dg, ok, sp, dp, st) == dg.DG_OK
    dst[:] = 0x5A
    assert _call(dg, ok, sp, dp, st, n=0) == dg.DG_OK and (dst == 0x5A).all()                     # n_frames = 0 does nothing
    D = dg.DgObsDesc
    bad = [D(0, 2, 0, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 0, 0, 0, 3, 0, 255, 1.0, 0.0, 0), D(17, 2, 0, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 17, 0, 0, 3, 0, 255, 1.0, 0.0, 0),
           D(2, 2, 3, 0, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 0xFFFFFFFF, 0, 3, 0, 255, 1.0, 0.0, 0),                       # unknown source
           D(2, 2, 2, 2, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 0, 1, 3, 0, 255, 1.0, 0.0, 0), D(2, 2, 1, 1, 3, 0, 255, 1.0, 0.0, 0),     # rule
           D(2, 2, 0, 0, 4, 0, 255, 1.0, 0.0, 0), D(2, 2, 0, 0, 0xFFFFFFFF, 0, 255, 1.0, 0.0, 0),                       # unknown dtype
           D(2, 2, 0, 0, 3, 0, 255, 1.0, 0.0, 1),                                                                       # reserved
           D(2, 2, 0, 0, 3, 5, 4, 1.0, 0.0, 0), D(2, 2, 0, 0, 3, -32769, 0, 1.0, 0.0, 0), D(2, 2, 0, 0, 3, 0, 32768, 1.0, 0.0, 0),   # clamp
           D(2, 2, 0, 0, 3, 0, 255, inf, 0.0, 0), D(2, 2, 0, 0, 3, 0, 255, nan, 0.0, 0), D(2, 2, 0, 0, 3, 0, 255, 1.0, -inf, 0), D(2, 2, 0, 0, 3, 0, 255, 1.0, nan, 0),
           D(2, 2, 0, 0, 0, 0, 255, 2.0, 0.0, 0), D(2, 2, 0, 0, 0, 0, 255, 1.0, 1.0, 0), D(2, 2, 0, 0, 0, -1, 255, 1.0, 0.0, 0), D(2, 2, 0, 0, 0, 0, 256, 1.0, 0.0, 0)]  # U8
    for d in bad:
        what = [getattr(d, f) for f, _ in d._fields_]
        assert L.dg_observed_size(8, 8, ctypes.byref(d), None, None, None, None) == dg.DG_ERR_INVALID, what
        assert _call(dg, d, sp, dp, st) == dg.DG_ERR_INVALID, what
        assert L.dg_last_error()
    assert _call(dg, D(2, 2, 2, 1, 0, 0, 255, 1.0, 0.0, 0), sp, dp, (16, 16, 4, 1)) == dg.DG_OK                         # (a good U8 / distance one)
    assert L.dg_observed_size(8, 8, None, None, None, None, None) == dg.DG_ERR_INVALID
    for args in ((None, sp, dp, st), (ok, None, dp, st), (ok, sp, None, st), (ok, sp, dp, None)):                       # a NULL argument
        assert _call(dg, *args) == dg.DG_ERR_INVALID
    for (w, h) in ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)):
        assert L.dg_observed_size(w, h, ctypes.byref(ok), None, None, None, None) == dg.DG_ERR_INVALID
        assert _call(dg, ok, sp, dp, st, W=w, H=h) == dg.DG_ERR_INVALID
    assert _call(dg, ok, sp, dp, st, n=-1) == dg.DG_ERR_INVALID
    # alignment: a distance source on an odd address; a dst off its element size; a colour source sits anywhere
    dist = D(2, 2, dg.DG_OBS_DISTANCE, dg.DG_PLANE_NEAREST, dg.DG_OBS_F16, -32768, 32767, 1.0, 0.0, 0)
    assert _call(dg, dist, P(src.ctypes.data + 1), dp, (16, 16, 4, 1)) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert _call(dg, dist, P(src.ctypes.data + 2), dp, (16, 16, 4, 1)) == dg.DG_OK
    assert _call(dg, dist, sp, P(dst.ctypes.data + 1), (16, 16, 4, 1)) == dg.DG_ERR_INVALID and b"aligned" in L.dg_last_error()
    assert _call(dg, ok, sp, P(dst.ctypes.data + 2), st) == dg.DG_ERR_INVALID
    assert _call(dg, ok, P(src.ctypes.data + 1), P(dst.ctypes.data + 4), st) == dg.DG_OK
    u8 = D(2, 2, 0, 0, 0, 0, 255, 1.0, 0.0, 0)
    assert _call(dg, u8, P(src.ctypes.data + 3), P(dst.ctypes.data + 1), st) == dg.DG_OK
    dst[:] = 0x5A
    for d in bad:
        _call(dg, d, sp, dp, st)
    assert (dst == 0x5A).all()                                                                                          # a refused call writes nothing
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    assert L.dg_observe_device(None, sp, 8, 8, 1, ctypes.byref(ok), dp, (ctypes.c_int64 * 4)(*st)) == dg.DG_ERR_INVALID
    assert L.dg_ctx_observe_kernel_ms(None, None) == dg.DG_ERR_INVALID


def test_the_stride_rule(dg):
    """8x8 RGB under 2x2: extents (n, 3, 4, 4)."""
    src = np.zeros(3 * 8 * 8 * 3, np.uint8)
    dst = np.zeros(1 << 16, np.float32)
    ok = dg.DgObsDesc(2, 2, dg.DG_OBS_RGB, 0, dg.DG_OBS_F32, -32768, 32767, 1.0, 0.0, 0)
    call = lambda st, n=3: _call(dg, ok, P(src.ctypes.data), P(dst.ctypes.data), st, n=n)
    accepted = [(48, 16, 4, 1), (48, 1, 12, 3), (100, 20, 5, 1), (480, 16, 4, 1), (48, 16, 1, 4), (1, 3, 9, 36), (3, 1, 9, 36), (1000, 300, 64, 16)]
    for st in accepted:
        assert call(st) == dg.DG_OK, st
    refused = [(48, 16, 4, 0), (48, 16, 0, 1), (48, 0, 4, 1), (0, 16, 4, 1),                   # a zero stride
               (48, 16, 4, -1), (48, 16, -4, 1), (-48, 16, 4, 1),                              # a negative stride
               (48, 16, 3, 1), (48, 15, 4, 1), (47, 16, 4, 1), (16, 16, 4, 1), (48, 16, 4, 4), (48, 1, 12, 2), (48, 2, 12, 3), (1, 1, 1, 1),
               (48, 16, 4, 2)]                                                                  # two elements would share an address
    for st in refused:
        assert call(st) == dg.DG_ERR_INVALID, st
        assert b"stride" in dg.lib().dg_last_error()
    # a dimension of extent 1 takes no part: one frame may have any frame stride >= 1, a 1x1 observation any row and column stride
    assert call((1, 16, 4, 1), n=1) == dg.DG_OK and call((0, 16, 4, 1), n=1) == dg.DG_ERR_INVALID
    one = dg.DgObsDesc(16, 16, dg.DG_OBS_GRAY, 0, dg.DG_OBS_F32, -32768, 32767, 1.0, 0.0, 0)
    assert _call(dg, one, P(src.ctypes.data), P(dst.ctypes.data), (1, 1, 1, 1), n=3) == dg.DG_OK
    assert _call(dg, one, P(src.ctypes.data), P(dst.ctypes.data), (1, 5, 7, 9), n=3) == dg.DG_OK
    assert call((1 << 62, 16, 4, 1)) == dg.DG_ERR_INVALID                                       # beyond any address


class StandIn:
    """What observe_into needs of a tensor, on host memory: shape, stride() in elements, data_ptr(), a dtype whose name ends right."""

    def __init__(self, array, dtype_name):
        self.a, self.dtype, self.shape = array, "torch." + dtype_name, array.shape

    def stride(self):
        return tuple(s // self.a.itemsize for s in self.a.strides)

    def data_ptr(self):
        return self.a.ctypes.data


def test_observe_into_checks_shape_and_dtype(dg):
    """observe_into refuses before it reaches the library, so a context-less object shows it: the C call would need a GPU."""
    d = dg.DgObsDesc(2, 2, dg.DG_OBS_RGB, 0, dg.DG_OBS_F16, -32768, 32767, 1.0, 0.0, 0)
    seen = []

    class Ctx:
        observe_into = dg.Context.observe_into

        def observe_device(self, *args):
            seen.append(args)

    good = StandIn(np.zeros((2, 3, 4, 4), np.float16), "float16")
    Ctx().observe_into(1234, 8, 8, 2, d, good)
    assert seen == [(1234, 8, 8, 2, d, good.data_ptr(), (48, 16, 4, 1))]
    view = StandIn(np.zeros((2, 5, 4, 6), np.float16)[:, 1:4, :, :4], "float16")              # a slice keeps its strides
    Ctx().observe_into(1234, 8, 8, 2, d, view)
    assert seen[-1][-1] == (120, 24, 6, 1) and seen[-1][-2] == view.data_ptr()
    for bad in (StandIn(np.zeros((2, 3, 4, 5), np.float16), "float16"), StandIn(np.zeros((3, 3, 4, 4), np.float16), "float16"),
                StandIn(np.zeros((2, 1, 4, 4), np.float16), "float16"), StandIn(np.zeros((2, 3, 4, 4), np.float32), "float32"),
                StandIn(np.zeros((2, 3, 4, 4), np.uint16), "bfloat16"), StandIn(np.zeros((2, 3, 16), np.float16), "float16")):
        with pytest.raises(ValueError):
            Ctx().observe_into(1234, 8, 8, 2, d, bad)
    assert len(seen) == 2


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_observed_size", "dg_observe_host", "dg_observe_device", "dg_ctx_observe_kernel_ms"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert (dg.DG_OBS_RGB, dg.DG_OBS_GRAY, dg.DG_OBS_DISTANCE) == (0, 1, 2) == (npo.RGB, npo.GRAY, npo.DISTANCE)
    assert (dg.DG_OBS_U8, dg.DG_OBS_F16, dg.DG_OBS_BF16, dg.DG_OBS_F32) == (0, 1, 2, 3) == npo.DTYPES
    assert b"ABI 4" in dg.lib().dg_version()
    assert ctypes.sizeof(dg.DgObsDesc) == 40
    for f in ("observed_size", "observe_host"):
        assert callable(getattr(dg, f))
    for f in ("observe_device", "observe_into", "observe_kernel_ms"):
        assert callable(getattr(dg.Context, f))
    src = open(os.path.join(ROOT, "doom-rust-renderer_amd", "__init__.py")).read()
    assert "import torch" not in src                                                           # the package itself never imports torch


def test_the_host_entry_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/observe/observe_host_main.cpp (its own main) with the host sources of the library, built with -fsanitize=address,undefined
    and run as a program: it checks its own results, and any sanitizer report fails it."""
    exe = tmp_path / "observe_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "observe", "observe_host_main.cpp")] +
                          [os.path.join(CSRC, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "observe_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
