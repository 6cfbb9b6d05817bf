"""GPU tier of the 2-D map view (dg_submit_map_views / dg_render_map_views): frames byte-equal to the numpy restatement (np_automap),
checksums of a 1 000-frame play-through, the slot machinery (async readback, replay, timing), layer invalidation by a new upload,
map and 3-D submissions sharing slots, the C++ mirror's render_map and the error returns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import np_automap as na
from test_automap_host import MAPS, SIZES, views_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1, K2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9)


def with_arrow(layer, mv, W, H, rv):
    """The restatement's frame: the linedef layer, then the arrow's three lines (drawn last, all yellow)."""
    img = layer.copy()
    arrow = na.rasterise(mv.arrow(W, H, *rv), W, H)
    hit = arrow.any(axis=2)
    img[hit] = arrow[hit]
    return img


@pytest.fixture(scope="module")
def maps(synth):
    return {k: f(synth) for k, f in MAPS.items()}


@pytest.mark.parametrize("name", list(MAPS))
def test_map_frames_equal_restatement(dg, maps, path1993, name):
    wad = maps[name]
    sc = dg.Scene(wad, "E1M1")
    mv = na.MapView(wad)
    pairs = views_for(mv, path1993)
    views = (dg.DgView * len(pairs))(*[v for v, _ in pairs])
    for W, H in SIZES:
        ctx = dg.Context(W, H, max_batch=len(pairs), slots=1)
        ctx.upload_scene(sc)
        out = ctx.render_map(views)
        layer = na.rasterise(mv.lines_for(W, H), W, H)
        for k, (_, rv) in enumerate(pairs):
            want = with_arrow(layer, mv, W, H, rv)
            assert np.array_equal(out[k], want), (name, W, H, k, int((out[k] != want).any(axis=2).sum()))
        ctx.close()
    sc.close()


def test_batches_of_1_9_and_max(dg, wad1993, path1993):
    sc = dg.Scene(wad1993, "E1M1")
    mv = na.MapView(wad1993)
    W, H, F = 320, 200, 24
    ctx = dg.Context(W, H, max_batch=F, slots=2)
    ctx.upload_scene(sc)
    layer = na.rasterise(mv.lines_for(W, H), W, H)
    for n, first in ((1, 5), (9, 100), (F, 700)):
        recs = path1993[first:first + n]
        out = ctx.render_map(dg.make_views(recs))
        for k in range(n):
            assert np.array_equal(out[k], with_arrow(layer, mv, W, H, na.path_view(recs[k]))), (n, k)
    ctx.close()


def _checksum_terms(d, i):
    with np.errstate(over="ignore"):
        m = (d.astype(np.uint64) ^ (i.astype(np.uint64) * K1)) * K2
        return m ^ (m >> np.uint64(32))


def test_campath_1000_frames_by_checksums(dg, wad1993, path1993):
    W, H = 1280, 800
    sc = dg.Scene(wad1993, "E1M1")
    mv = na.MapView(wad1993)
    ctx = dg.Context(W, H, max_batch=1000, slots=1)
    ctx.upload_scene(sc)
    ctx.submit_map(0, dg.make_views(path1993))
    got = ctx.frame_checksums(0, 0, 1000)
    t = ctx.timing(0)
    assert t["front_end"] == dg.DG_FE_MAP and t["n_frames"] == 1000 and t["setup_ms"] > 0 and t["raster_ms"] > 0
    layer = na.rasterise(mv.lines_for(W, H), W, H)
    flat = layer.reshape(-1)
    dwords = flat.view("<u4")
    base = np.uint64(dg.frame_checksum(layer))
    for f in range(1000):
        arrow = na.rasterise(mv.arrow(W, H, *na.path_view(path1993[f])), W, H)
        px = np.nonzero(arrow.reshape(-1, 3).any(axis=1))[0]
        touched = np.unique(np.concatenate([(3 * px + j) // 4 for j in range(3)]))
        new = flat.copy()
        for j in range(3):
            new[3 * px + j] = arrow.reshape(-1, 3)[px, j]
        with np.errstate(over="ignore"):
            want = base - _checksum_terms(dwords[touched], touched).sum(dtype=np.uint64) + \
                _checksum_terms(new.view("<u4")[touched], touched).sum(dtype=np.uint64)
        assert got[f] == want, f
    ctx.close()


def test_readback_async_replay_and_timing(dg, wad1993, path1993):
    W, H, n = 640, 400, 9
    sc = dg.Scene(wad1993, "E1M1")
    mv = na.MapView(wad1993)
    ctx = dg.Context(W, H, max_batch=16, slots=2)
    ctx.upload_scene(sc)
    layer = na.rasterise(mv.lines_for(W, H), W, H)
    recs = path1993[200:200 + n]
    want = np.stack([with_arrow(layer, mv, W, H, na.path_view(r)) for r in recs])
    fallbacks = ctx.fallbacks()
    ctx.submit_map(1, dg.make_views(recs))
    host = dg.lib().dg_alloc_host(n * 3 * W * H)
    try:
        ctx.readback_async(1, 0, n, host)
        ctx.wait(1)
        got = np.ctypeslib.as_array((ctypes.c_uint8 * (n * 3 * W * H)).from_address(host)).reshape(n, H, W, 3).copy()
    finally:
        dg.lib().dg_free_host(host)
    assert np.array_equal(got, want)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP and t["setup_ms"] > 0            # this submission built the layer
    sums = ctx.frame_checksums(1, 0, n)
    assert list(sums) == [dg.frame_checksum(w) for w in want]
    # a second submission reuses the layer; a replay re-runs the per-frame kernels only
    ctx.submit_map(0, dg.make_views(recs[::-1]))
    assert ctx.timing(0)["setup_ms"] == 0.0
    assert np.array_equal(ctx.readback(0, 0, n), want[::-1])
    fb = ctx.framebuffer_ptr(1)
    ctx.replay(1)
    ctx.wait(1)
    t = ctx.timing(1)
    assert t["front_end"] == dg.DG_FE_MAP and t["setup_ms"] == 0.0 and t["raster_ms"] > 0 and t["total_ms"] == t["raster_ms"]
    assert ctx.framebuffer_ptr(1) == fb and list(ctx.frame_checksums(1, 0, n)) == list(sums)
    assert np.array_equal(ctx.readback(1, 0, n), want)
    assert ctx.fallbacks() == fallbacks
    ctx.close()


def test_second_upload_invalidates_the_layer(dg, maps, path1993):
    W, H = 320, 200
    ctx = dg.Context(W, H, max_batch=4, slots=1)
    recs = path1993[:4]
    for name in ("synth1993", "polygon1200", "synth1993"):
        sc = dg.Scene(maps[name], "E1M1")
        mv = na.MapView(maps[name])
        ctx.upload_scene(sc)
        out = ctx.render_map(dg.make_views(recs))
        assert ctx.timing(0)["setup_ms"] > 0
        layer = na.rasterise(mv.lines_for(W, H), W, H)
        for k in range(4):
            assert np.array_equal(out[k], with_arrow(layer, mv, W, H, na.path_view(recs[k]))), (name, k)
    ctx.close()


@pytest.mark.parametrize("front_end", [0, 1, 2, 3])
def test_map_and_3d_submissions_share_slots(dg, oracle, wad1993, path1993, front_end):
    W, H = 320, 200
    sc = dg.Scene(wad1993, "E1M1")
    osc = oracle.Scene(wad1993, "e1m1")
    mv = na.MapView(wad1993)
    idx = [0, 100, 297, 323, 500, 623, 728, 900]
    recs = path1993[idx]
    want3d = [dg.frame_checksum(osc.render(W, H, r)) for r in recs]
    layer = na.rasterise(mv.lines_for(W, H), W, H)
    wantmap = [dg.frame_checksum(with_arrow(layer, mv, W, H, na.path_view(r))) for r in recs]
    ctx = dg.Context(W, H, max_batch=8, slots=2, front_end=front_end)
    ctx.upload_scene(sc)
    v = dg.make_views(recs)
    # one slot: 3-D, map, 3-D
    ctx.submit(0, v)
    assert list(ctx.frame_checksums(0, 0, 8)) == want3d
    ctx.submit_map(0, v)
    assert list(ctx.frame_checksums(0, 0, 8)) == wantmap
    ctx.submit(0, v)
    assert list(ctx.frame_checksums(0, 0, 8)) == want3d
    assert ctx.timing(0)["front_end"] != dg.DG_FE_MAP
    # two slots, interleaved without waiting in between
    for first, second in ((ctx.submit, ctx.submit_map), (ctx.submit_map, ctx.submit)):
        first(0, v)
        second(1, v)
        ctx.wait(0)
        ctx.wait(1)
        a, b = list(ctx.frame_checksums(0, 0, 8)), list(ctx.frame_checksums(1, 0, 8))
        assert (a, b) == ((want3d, wantmap) if first == ctx.submit else (wantmap, want3d))
    ctx.close()


MIRROR_SRC = r'''
#include "doom-rust-renderer_amd/csrc/doomgpu.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
int main(int argc, char **argv) {
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    doom::World world(wad, "e1m1");
    doom::Device dev(W, H);
    dev.upload(world);
    doom::Player pl = world.player_start();
    pl.angle += 0.7f;
    doom::Pixels pixels(W, H);
    doom::Renderer(pixels, world, pl, 0.0f, dev).render_map();
    std::FILE *out = std::fopen(argv[4], "wb");
    std::fwrite(pixels.pixels.data(), 1, pixels.pixels.size(), out);
    std::fclose(out);
    std::printf("%a %a %a\n", pl.position.x, pl.position.y, pl.angle);
    return 0;
}
'''


def test_cpp_mirror_render_map(dg, wad1993, tmp_path):
    src, exe, wadf, outf = tmp_path / "m.cpp", tmp_path / "m", tmp_path / "map.wad", tmp_path / "frame.bin"
    src.write_text(MIRROR_SRC)
    wadf.write_bytes(wad1993)
    libdir = os.path.join(ROOT, "doom-rust-renderer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", ROOT, str(src), "-o", str(exe), os.path.join(libdir, "libdoomgpu.so"), "-Wl,-rpath," + libdir])
    W, H = 320, 200
    r = subprocess.run([str(exe), str(wadf), str(W), str(H), str(outf)], capture_output=True, text=True, timeout=120, check=True)
    x, y, a = (np.float32(float.fromhex(t)) for t in r.stdout.split())
    mv = na.MapView(wad1993)
    want = mv.render(W, H, na.libm_view(x, y, a))
    assert np.array_equal(np.fromfile(outf, dtype=np.uint8).reshape(H, W, 3), want)


def test_error_returns(dg, wad1993):
    L = dg.lib()
    sc = dg.Scene(wad1993, "E1M1")
    v = (dg.DgView * 4)(*[dg.DgView(1000.0, 1000.0, 0.5, 0, 0, 0, 0, 0, 0, 0)] * 4)
    ctx = dg.Context(320, 200, max_batch=3, slots=1)
    assert L.dg_submit_map_views(ctx._h, 0, v, 1) == dg.DG_ERR_INVALID             # no scene uploaded
    ctx.upload_scene(sc)
    assert L.dg_submit_map_views(ctx._h, 0, v, 4) == dg.DG_ERR_CAPACITY            # n > max_batch
    assert L.dg_submit_map_views(ctx._h, 0, v, 0) == dg.DG_ERR_CAPACITY
    assert L.dg_submit_map_views(ctx._h, 1, v, 1) == dg.DG_ERR_INVALID             # slot out of range
    assert L.dg_render_map_views(ctx._h, None, 1, None) == dg.DG_ERR_INVALID
    far = (dg.DgView * 1)(dg.DgView(1e9, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0))
    assert L.dg_submit_map_views(ctx._h, 0, far, 1) == dg.DG_ERR_INVALID           # arrow beyond +-2^24
    ctx.render_map((dg.DgView * 3)(*v[:3]))                                         # still usable
    ctx.close()
    for W, H in ((39, 40), (40, 39), (16, 16)):
        small = dg.Context(W, H, max_batch=1, slots=1)
        small.upload_scene(sc)
        assert L.dg_submit_map_views(small._h, 0, v, 1) == dg.DG_ERR_INVALID
        assert L.dg_render_map_views(small._h, v, 1, None) == dg.DG_ERR_INVALID
        small.close()
