"""CPU tier of the band kernels' extents: the launch plan of launch_reduce, launch_plane_reduce and launch_observe
restated in Python (tests/extent_cases.py) against the constants of the project's own headers (tests/extents/plan_check.cpp); the shape
table against the classes of launch it has to reach; the inputs of the cases past 2^32; and the host paths (dg_reduce_host,
dg_reduce_planes_host, dg_observe_host, dg_seen_lines_host), which have no runs, at every shape of the table against the numpy models,
so that a failure of tests/test_extents_gpu.py points at a kernel and not at a model."""
import os
import subprocess

import numpy as np
import pytest

import explored_cases as xc
import extent_cases as ec
import np_explored as ne
import np_observe as npo
import np_plane_reduce as npp
import np_reduce as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_IDS = [ec.shape_id(s) for s in ec.SHAPES]


def test_the_plan_has_the_constants_of_the_headers(tmp_path):
    """tests/extents/plan_check.cpp prints REDUCE_SPAN, PLANE_REDUCE_SPAN and both px_per_wg for fx = 1..16 from csrc/reduce_kernels.hpp
    and csrc/plane_reduce_kernels.hpp: the Python plan has the same numbers, so the shape table cannot drift from the constants."""
    exe = tmp_path / "plan_check"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "extents", "plan_check.cpp"), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    assert lines[0] == f"spans {ec.REDUCE_SPAN} {ec.PLANE_REDUCE_SPAN} {ec.LANES} {ec.LANES} 16"
    assert lines[1:17] == [f"{fx} {ec.reduce_px_per_wg(fx)} {ec.plane_reduce_px_per_wg(fx)}" for fx in range(1, 17)]
    assert max(fx for fx, _ in npr.FACTORS) <= 16


def test_the_plan_on_known_rows():
    """The run lengths the issue of these tests was written from, and a few plans by hand."""
    assert [ec.reduce_px_per_wg(fx) for fx in (1, 2, 3, 4, 7, 16)] == [1360, 680, 453, 340, 194, 85]
    assert [ec.plane_reduce_px_per_wg(fx) for fx in (1, 2, 3, 4, 7, 16)] == [2041, 1020, 680, 510, 291, 127]
    assert ec.launch_plan("colour", 1280, 2) == {"pieces": True, "per": 680, "runs": [(640, 0)], "short_box": False}      # the widest row before
    assert ec.launch_plan("column", 1280, 1)["runs"] == [(1280, 0)]
    assert ec.launch_plan("colour", 1360, 3) == {"pieces": True, "per": 453, "runs": [(453, 0), (1, 13)], "short_box": True}
    assert ec.launch_plan("colour", 1360, 7)["runs"] == [(194, 0), (1, 10)]
    assert ec.launch_plan("colour", 2720, 3, base_off=1)["runs"] == [(453, 0), (453, 0), (1, 0)]
    assert ec.launch_plan("column", 2048, 1) == {"pieces": True, "per": 2041, "runs": [(2041, 0), (7, 1)], "short_box": False}
    assert ec.launch_plan("column", 2720, 7)["runs"] == [(291, 0), (98, 5)]
    assert ec.launch_plan("column", 2042, 1) == {"pieces": False, "per": 2041, "runs": [(2041, 0), (1, 0)], "short_box": False}
    assert ec.launch_plan("point", 513, 1)["runs"] == [(256, 0), (256, 0), (1, 0)]
    # every run fits the workgroup's span, the pieces in front of it included
    for fx in range(1, 17):
        for W in (1, 1360, 4113, 16383, 16384):
            assert all(3 * fx * n + off <= ec.REDUCE_SPAN for n, off in ec.launch_plan("colour", W, fx)["runs"])
            assert all(fx * n + off <= ec.PLANE_REDUCE_SPAN for n, off in ec.launch_plan("column", W, fx)["runs"])


def test_the_shape_table_reaches_every_launch_class():
    got, need = ec.reached(), ec.required_classes()
    assert need <= got, sorted(need - got)
    # what ran before these tests reaches no run but the first: the widest sources of the older grids
    for W in (1280, 320, 131):
        for fx, _ in npr.FACTORS:
            assert len(ec.launch_plan("colour", W, fx)["runs"]) == 1 and len(ec.launch_plan("column", W, fx)["runs"]) == 1
    assert len(ec.cases()) == len(ec.SHAPES) * len(npr.FACTORS)


def test_the_frame_counts_and_the_sizes_past_2_to_the_32():
    assert ec.FRAME_COUNTS == (65535, 65536, 131070, 131071)
    for entry, (W, H, bpp) in ec.BIG_SOURCES.items():
        fb = W * H * bpp
        f, wrapped = ec.first_frame_behind(fb)
        n = ec.big_frames(fb)
        assert n % ec.K_BASE == 0 and ec.K_BASE % 2 == 1
        assert ec.TWO32 % fb != 0 and ec.TWO32 < n * fb < ec.TWO32 + 8 * fb and f + 1 < n and 0 < wrapped < fb, entry
        assert n * fb < 4.4e9, entry
    base = np.arange(3 * 5000, dtype=np.uint32).astype(np.uint8).reshape(3, 5000)
    assert ec.wrapped_bytes_differ(base, 7, 123) and not ec.wrapped_bytes_differ(base, 6, 3 * 5000 * 4)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=SHAPE_IDS)
def test_reduce_host_at_every_table_shape(dg, shape):
    W, H0, _ = shape
    for fx, fy in npr.FACTORS:
        frames = ec.colour_frames(W, ec.height_of(H0, fy))
        for fmt in (npr.RGB24, npr.GRAY8):
            assert np.array_equal(dg.reduce_host(frames, (fx, fy, fmt)), npr.reduce(frames, fx, fy, fmt)), (fx, fy, fmt)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=SHAPE_IDS)
def test_reduce_planes_host_at_every_table_shape(dg, shape):
    W, H0, _ = shape
    for fx, fy in npr.FACTORS:
        planes = ec.plane_sources(W, ec.height_of(H0, fy), fx, fy)
        for rule in (npp.POINT, npp.NEAREST):
            got, want = dg.reduce_planes_host((fx, fy, rule), **planes), npp.reduce(rule, fx, fy, **planes)
            assert set(got) == set(want) == set(npp.NAMES)
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (fx, fy, rule, k)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=SHAPE_IDS)
def test_observe_host_at_every_table_shape(dg, shape):
    W, H0, _ = shape
    k = 0
    for fx, fy in npr.FACTORS:
        H = ec.height_of(H0, fy)
        for source, rule in npo.KINDS:
            src = npo.sources(source, 3, W, H, fx, fy)
            v = npo.values(source, rule, fx, fy, src)
            for dtype in npo.DTYPES:
                maps = list(npo.maps_for(dtype).values())
                scale, bias, lo, hi = maps[k % len(maps)]
                k += 1
                got = dg.observe_host(src, dg.DgObsDesc(fx, fy, source, rule, dtype, lo, hi, float(scale), float(bias), 0))
                assert np.array_equal(got.view(npo.BITS[dtype]), npo.convert(v, dtype, lo, hi, scale, bias)), (fx, fy, source, rule, dtype)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=SHAPE_IDS)
def test_seen_lines_host_at_every_table_shape(dg, wad1993, shape):
    W, H0, _ = shape
    ex, scene = ne.Explored(wad1993), dg.Scene(wad1993, "e1m1")
    names, ids, cls = xc.stacked(xc.synthetic_planes(ex, W, ec.height_of(H0, 1)))
    assert np.array_equal(dg.seen_lines_host(scene, ids, cls), ex.seen(ids, cls))
    scene.close()


def test_the_fast_seen_model_is_np_explored(wad1993):
    """The cases past one launch hold 131 071 frames of a few pixels against ec.seen_rows, a vectorised form of np_explored.Explored.seen
    (which walks frame by frame): the two agree on random planes."""
    ex = ne.Explored(wad1993)
    for (W, H) in ec.CHUNK_SHAPES["seen"]:
        ids, cls = ec.random_labels(500, H, W, len(ex.seg_line), seed=3)
        assert (cls == 1).any() and (ids >= len(ex.seg_line)).any()
        assert np.array_equal(ec.seen_rows(ex, ids, cls), ex.seen(ids, cls))
