"""CPU tier of the reduced-size frames: dg_reduce_host and dg_reduced_size against the numpy restatement
(np_reduce), byte for byte, over the grid of sizes, box sizes, formats, frame counts and contents both tiers share; the contract's
errors; and the multiply-high that replaces the division, exhaustively (tests/reduce/rcp_check.cpp over csrc/reduce_core.h, and the
same claim in numpy)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import np_reduce as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_reduce_host_equals_the_model(dg, size, factor):
    (W, H), (fx, fy) = size, factor
    for kind in npr.CONTENTS:
        frames = npr.content(kind, 3, W, H)
        for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
            want = npr.reduce(frames, fx, fy, fmt)
            for n in (1, 3):
                got = dg.reduce_host(frames[:n], (fx, fy, fmt))
                assert got.shape == want[:n].shape and got.dtype == np.uint8
                assert np.array_equal(got, want[:n]), (kind, fmt, n, np.argwhere(got != want[:n])[:4])
            if kind == "ones":
                assert (want == 255).all()                      # the largest sum, 255 * n, does not wrap; gray of white is white
            if kind == "zeros":
                assert not want.any()
            if kind == "checker" and (fx, fy) == (2, 2):
                assert (want[:, :H // 2, :W // 2] == 128).all()  # every whole 2x2 box is x.5: halves go up
        if (fx, fy) == (1, 1):
            assert np.array_equal(dg.reduce_host(frames, (1, 1)), frames)   # a copy


def test_edge_boxes_divide_by_their_own_pixel_count(dg):
    """Only the last row and column are 255: a short box at the edge that is all 255 must give 255, which it does only when it is
    divided by the pixels that exist."""
    W, H = 131, 67
    out = dg.reduce_host(npr.content("last", 1, W, H), (7, 3))
    assert out.shape == (1, 23, 19, 3)
    assert (out[0, -1, :, :] == 255).all()                      # 67 = 22 * 3 + 1: the last band is the one row of 255
    assert out[0, 0, -1, 0] == (2 * 255 * 3 + 15) // 30         # 131 = 18 * 7 + 5: three of the 15 pixels of that box are 255
    assert out[0, 0, 0, 0] == 0


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reduced_size(dg, size):
    W, H = size
    for fx, fy in npr.FACTORS:
        for fmt in (dg.DG_REDUCE_RGB24, dg.DG_REDUCE_GRAY8):
            assert dg.reduced_size(W, H, (fx, fy, fmt)) == npr.reduced_size(W, H, fx, fy, fmt)
    d = dg.DgReduceDesc(2, 2, 0, 0)
    assert dg.lib().dg_reduced_size(W, H, ctypes.byref(d), None, None, None) == dg.DG_OK     # every output is optional


def test_contract_errors(dg):
    L = dg.lib()
    src = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    dst = np.zeros(64, dtype=np.uint8)
    sp, dp = src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p)
    ok = dg.DgReduceDesc(2, 2, dg.DG_REDUCE_RGB24, 0)
    assert L.dg_reduce_host(sp, 4, 4, 1, ctypes.byref(ok), dp) == dg.DG_OK
    assert L.dg_reduce_host(sp, 4, 4, 0, ctypes.byref(ok), dp) == dg.DG_OK
    bad = [dg.DgReduceDesc(0, 2, 0, 0), dg.DgReduceDesc(2, 0, 0, 0), dg.DgReduceDesc(17, 2, 0, 0), dg.DgReduceDesc(2, 17, 0, 0),
           dg.DgReduceDesc(2, 2, 2, 0), dg.DgReduceDesc(2, 2, 0xFFFFFFFF, 0), dg.DgReduceDesc(2, 2, 0, 1)]
    for d in bad:
        assert L.dg_reduced_size(4, 4, ctypes.byref(d), None, None, None) == dg.DG_ERR_INVALID, (d.fx, d.fy, d.format, d.reserved)
        assert L.dg_reduce_host(sp, 4, 4, 1, ctypes.byref(d), dp) == dg.DG_ERR_INVALID
        assert L.dg_last_error()
    assert not dst.any()                                         # a refused call writes nothing
    assert L.dg_reduced_size(4, 4, None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduced_size(0, 4, ctypes.byref(ok), None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduced_size(4, -1, ctypes.byref(ok), None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduce_host(None, 4, 4, 1, ctypes.byref(ok), dp) == dg.DG_ERR_INVALID
    assert L.dg_reduce_host(sp, 4, 4, 1, ctypes.byref(ok), None) == dg.DG_ERR_INVALID
    assert L.dg_reduce_host(sp, 4, 4, 1, None, dp) == dg.DG_ERR_INVALID
    assert L.dg_reduce_host(sp, 4, 4, -1, ctypes.byref(ok), dp) == dg.DG_ERR_INVALID
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    for fn in (L.dg_readback_reduced, L.dg_readback_reduced_async):
        assert fn(None, 0, 0, 0, ctypes.byref(ok), dp) == dg.DG_ERR_INVALID
    assert L.dg_reduce_device(None, sp, 4, 4, 1, ctypes.byref(ok), dp) == dg.DG_ERR_INVALID
    assert L.dg_ctx_reduce_kernel_ms(None, None) == dg.DG_ERR_INVALID


def test_multiply_high_equals_the_division_exhaustively():
    """mul_hi(x, ceil(2^32 / 2n)) == x // 2n for every n in 1..256 and every x in [0, 2*255*n + n]: 16.8 M cases, in numpy."""
    cases = 0
    for n in range(1, 257):
        x = np.arange(0, 2 * 255 * n + n + 1, dtype=np.uint64)
        m = np.uint64(-((-1 << 32) // (2 * n)))
        assert int(m) == ((1 << 32) + 2 * n - 1) // (2 * n) and int(m) < 1 << 32
        assert np.array_equal((x * m) >> np.uint64(32), x // np.uint64(2 * n)), n
        cases += x.size
    assert cases == sum(511 * n + 1 for n in range(1, 257))


def test_reduce_core_rounded_divide_exhaustively(tmp_path):
    """The same claim about the code itself: reduce_rcp and reduce_round of csrc/reduce_core.h, which dg_reduce_host and the kernel share."""
    exe = tmp_path / "rcp_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "reduce", "rcp_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout == "ok %d\n" % sum(511 * n + 1 for n in range(1, 257)), r.stdout + r.stderr


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_reduced_size", "dg_reduce_host", "dg_readback_reduced", "dg_readback_reduced_async", "dg_reduce_device", "dg_ctx_reduce_kernel_ms"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert dg.lib().dg_version() == b"doomgpu 0.6 (gfx950; ABI 4)"
    assert ctypes.sizeof(dg.DgReduceDesc) == 16
