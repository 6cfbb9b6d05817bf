"""CPU tier of the reduced depth and label planes: dg_reduce_planes_host and dg_plane_reduced_size against the
numpy restatement (np_plane_reduce), byte for byte.

  grid          np_reduce.SIZES x np_reduce.FACTORS x both rules x 1 and 3 frames x four distance contents (full-range random, all equal,
                a small value only in the last row and column, each box's minimum at its last pixel); id names the source pixel, kind and
                cls follow from it, so a wrong tie-break or a plane sampled at another pixel shows
  pairs         any source / destination pair left out
  whole frames  4 path frames of the light map at 160x100 through dg_build_lists_owners -> dg_bundle_lists_host -> dg_reduce_planes_host
  errors        every error return of the contract
  stand-alone   tests/plane_reduce/plane_reduce_host_main.cpp under AddressSanitizer + UBSan, as a program
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import np_plane_reduce as npp
import np_reduce as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
RULES = (npp.POINT, npp.NEAREST)


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {len(bad)} {k} entries differ, first at {bad[0].tolist()}: got {got[k][tuple(bad[0])]} model {want[k][tuple(bad[0])]}"


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_reduce_planes_host_equals_the_model(dg, size, factor):
    (W, H), (fx, fy) = size, factor
    tracer = npp.tracer_planes(3, W, H)
    if W * H <= 65536:
        assert np.unique(tracer["id"][0]).size == W * H              # the id names its pixel
    for kind in npp.CONTENTS:
        planes = dict(tracer, distance=npp.distance_content(kind, 3, W, H, fx, fy))
        if kind == "random" and W * H > 1:
            assert planes["distance"].min() == -32768 and planes["distance"].max() == 32767
        for rule in RULES:
            want = npp.reduce(rule, fx, fy, **planes)
            for n in (1, 3):
                got = dg.reduce_planes_host((fx, fy, rule), **{k: v[:n] for k, v in planes.items()})
                _same(got, {k: v[:n] for k, v in want.items()}, (kind, rule, n))
            if (fx, fy) == (1, 1):
                _same(want, planes, "1x1 is a copy")
            if kind == "boxlast" and rule == npp.NEAREST:            # the representative is the last pixel of the box that exists
                oW, oH = npp.reduced_size(W, H, fx, fy)
                ys = np.minimum(H, (np.arange(oH) + 1) * fy) - 1
                xs = np.minimum(W, (np.arange(oW) + 1) * fx) - 1
                assert np.array_equal(want["id"][0], ((ys[:, None] * W + xs[None, :]) & 0xFFFF).astype(np.uint16))
            if kind == "equal" and rule == npp.NEAREST:              # every tie: the first pixel of the box
                oW, oH = npp.reduced_size(W, H, fx, fy)
                assert np.array_equal(want["id"][0], (((np.arange(oH) * fy)[:, None] * W + (np.arange(oW) * fx)[None, :]) & 0xFFFF).astype(np.uint16))


def test_edge_boxes_see_only_the_pixels_that_exist(dg):
    """131 = 18*7 + 5 and 67 = 22*3 + 1: the only small values sit in the last row and column, so every box at the right or bottom edge
    must take one of them, and its representative is inside the frame."""
    W, H, fx, fy = 131, 67, 7, 3
    planes = dict(npp.tracer_planes(1, W, H), distance=npp.distance_content("last", 1, W, H, fx, fy))
    got = dg.reduce_planes_host((fx, fy, npp.NEAREST), **planes)
    assert got["distance"].shape == (1, 23, 19)
    assert (got["distance"][0, -1, :] == -7).all() and (got["distance"][0, :, -1] == -7).all() and (got["distance"][0, :-1, :-1] == 1000).all()
    assert got["id"][0, 0, -1] == 130 and got["id"][0, -1, 0] == 66 * W and got["id"][0, 0, 0] == 0
    pt = dg.reduce_planes_host((fx, fy, npp.POINT), **planes)
    assert pt["id"][0, -1, -1] == 66 * W + 129 and pt["id"][0, 0, 0] == 1 * W + 3     # min(W-1, 18*7 + 3), min(H-1, 22*3 + 1)


def test_any_pair_may_be_left_out(dg):
    W, H, fx, fy = 80, 50, 4, 5
    planes = dict(npp.tracer_planes(3, W, H), distance=npp.distance_content("random", 3, W, H, fx, fy))
    for r in range(1, 5):
        for names in itertools.combinations(npp.NAMES, r):
            sub = {k: planes[k] for k in names}
            for rule in RULES:
                if rule == npp.NEAREST and "distance" not in names:
                    with pytest.raises(dg.DoomGpuError) as e:
                        dg.reduce_planes_host((fx, fy, rule), **sub)
                    assert e.value.code == dg.DG_ERR_INVALID
                else:
                    _same(dg.reduce_planes_host((fx, fy, rule), **sub), npp.reduce(rule, fx, fy, **sub), (names, rule))


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_reduced_size(dg, size):
    W, H = size
    for fx, fy in npr.FACTORS:
        for rule in RULES:
            assert dg.plane_reduced_size(W, H, (fx, fy, rule)) == npp.reduced_size(W, H, fx, fy)
    d = dg.DgPlaneReduceDesc(2, 2, 0, 0)
    assert dg.lib().dg_plane_reduced_size(W, H, ctypes.byref(d), None, None) == dg.DG_OK      # every output is optional


def test_contract_errors(dg):
    L = dg.lib()
    W = H = 4
    src = {"distance": np.zeros((1, H, W), np.int16), "kind": np.zeros((1, H, W), np.uint8), "id": np.zeros((1, H, W), np.uint16), "cls": np.zeros((1, H, W), np.uint8)}
    dst = {k: np.full((1, 2, 2), 77, v.dtype) for k, v in src.items()}
    sp = [src[k].ctypes.data_as(P) for k in npp.NAMES]
    dp = [dst[k].ctypes.data_as(P) for k in npp.NAMES]
    ok = dg.DgPlaneReduceDesc(2, 2, dg.DG_PLANE_NEAREST, 0)
    assert L.dg_reduce_planes_host(W, H, 0, ctypes.byref(ok), *sp, *dp) == dg.DG_OK
    assert all((v == 77).all() for v in dst.values())                 # n_frames = 0 writes nothing
    bad = [dg.DgPlaneReduceDesc(0, 2, 0, 0), dg.DgPlaneReduceDesc(2, 0, 0, 0), dg.DgPlaneReduceDesc(17, 2, 0, 0), dg.DgPlaneReduceDesc(2, 17, 1, 0),
           dg.DgPlaneReduceDesc(2, 2, 2, 0), dg.DgPlaneReduceDesc(2, 2, 0xFFFFFFFF, 0), dg.DgPlaneReduceDesc(2, 2, 0, 1), dg.DgPlaneReduceDesc(2, 2, 1, 1)]
    for d in bad:
        assert L.dg_plane_reduced_size(W, H, ctypes.byref(d), None, None) == dg.DG_ERR_INVALID, (d.fx, d.fy, d.rule, d.reserved)
        assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(d), *sp, *dp) == dg.DG_ERR_INVALID
        assert L.dg_last_error()
    assert L.dg_plane_reduced_size(W, H, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_reduce_planes_host(W, H, 1, None, *sp, *dp) == dg.DG_ERR_INVALID
    for (w, h) in ((0, 4), (4, 0), (-1, 4), (16385, 4), (4, 16385)):
        assert L.dg_plane_reduced_size(w, h, ctypes.byref(ok), None, None) == dg.DG_ERR_INVALID
        assert L.dg_reduce_planes_host(w, h, 1, ctypes.byref(ok), *sp, *dp) == dg.DG_ERR_INVALID
    assert L.dg_plane_reduced_size(16384, 16384, ctypes.byref(ok), None, None) == dg.DG_OK
    assert L.dg_reduce_planes_host(W, H, -1, ctypes.byref(ok), *sp, *dp) == dg.DG_ERR_INVALID
    for k in range(4):                                                # a source without its destination, and the reverse
        s2, d2 = list(sp), list(dp)
        d2[k] = None
        assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(ok), *s2, *d2) == dg.DG_ERR_INVALID
        s2, d2 = list(sp), list(dp)
        s2[k] = None
        assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(ok), *s2, *d2) == dg.DG_ERR_INVALID
    no_d = ([None] + sp[1:], [None] + dp[1:])
    assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(ok), *no_d[0], *no_d[1]) == dg.DG_ERR_INVALID      # NEAREST needs the distance plane
    assert all((v == 77).all() for v in dst.values())                 # a refused call writes nothing
    assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(dg.DgPlaneReduceDesc(2, 2, dg.DG_PLANE_POINT, 0)), *no_d[0], *no_d[1]) == dg.DG_OK
    assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(ok), *([None] * 8)) == dg.DG_ERR_INVALID
    assert L.dg_reduce_planes_host(W, H, 1, ctypes.byref(dg.DgPlaneReduceDesc(2, 2, dg.DG_PLANE_POINT, 0)), *([None] * 8)) == dg.DG_OK
    # the calls that take a ctx refuse a NULL one before they touch a GPU
    assert L.dg_reduce_planes_device(None, W, H, 1, ctypes.byref(ok), *sp, *dp) == dg.DG_ERR_INVALID
    assert L.dg_ctx_plane_reduce_kernel_ms(None, None) == dg.DG_ERR_INVALID
    for fn in (L.dg_readback_planes_reduced, L.dg_readback_planes_reduced_async):
        assert fn(None, 0, 0, 0, ctypes.byref(ok), None, None, None, None, None) == dg.DG_ERR_INVALID


@pytest.fixture(scope="module")
def map_frames(dg, wad1993, path1993):
    """The four planes of 4 path frames of the light map at 160x100: dg_build_lists_owners -> dg_bundle_lists_host."""
    W, H = 160, 100
    sc = dg.Scene(wad1993, "e1m1")
    views = dg.make_views(path1993[[100, 297, 623, 728]])
    out = {k: np.empty((4, H, W), dtype=npp.DTYPES[k]) for k in npp.NAMES}
    for i in range(4):
        fl, owners = sc.build_lists_owners(W, H, views[i])
        d, k, ids, cls, _ = dg.bundle_lists_host(sc, W, H, (dg.DgFrameLists * 1)(fl), [owners], boxes=False)
        out["distance"][i], out["kind"][i], out["id"][i], out["cls"][i] = d[0], k[0], ids[0], cls[0]
    sc.close()
    return W, H, out


@pytest.mark.parametrize("factor", [(4, 4), (5, 3)], ids=lambda f: f"{f[0]}x{f[1]}")
def test_whole_frames_of_the_light_map(dg, map_frames, factor):
    W, H, planes = map_frames
    fx, fy = factor
    assert {1, 2, 3} <= set(np.unique(planes["kind"]).tolist()) and {1, 2, 3, 4} <= set(np.unique(planes["cls"]).tolist())
    got = {}
    for rule in RULES:
        got[rule] = dg.reduce_planes_host((fx, fy, rule), **planes)
        _same(got[rule], npp.reduce(rule, fx, fy, **planes), (factor, rule))
    # the frames exercise the rule: NEAREST differs from POINT, and some box's representative is not its first pixel
    assert any((got[npp.NEAREST][k] != got[npp.POINT][k]).any() for k in npp.NAMES)
    ys, xs = npp.representatives(npp.NEAREST, 4, W, H, fx, fy, planes["distance"])
    oW, oH = npp.reduced_size(W, H, fx, fy)
    assert ((ys != (np.arange(oH) * fy)[None, :, None]) | (xs != (np.arange(oW) * fx)[None, None, :])).any()
    # every output pixel describes one real source pixel: the four values are those of the representative
    f = np.arange(4)[:, None, None]
    for k in npp.NAMES:
        assert np.array_equal(got[npp.NEAREST][k], planes[k][f, ys, xs])


def test_new_declarations_are_exported_and_bound(dg):
    names = ["dg_plane_reduced_size", "dg_reduce_planes_host", "dg_reduce_planes_device", "dg_ctx_plane_reduce_kernel_ms", "dg_readback_planes_reduced",
             "dg_readback_planes_reduced_async"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert (dg.DG_PLANE_POINT, dg.DG_PLANE_NEAREST) == (0, 1) == (npp.POINT, npp.NEAREST)
    assert b"ABI 4" in dg.lib().dg_version()
    assert ctypes.sizeof(dg.DgPlaneReduceDesc) == 16


def test_the_host_entry_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/plane_reduce/plane_reduce_host_main.cpp (its own main, the C-ABI alone) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: it checks its own results, and any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "plane_reduce_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "plane_reduce", "plane_reduce_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "plane_reduce_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
