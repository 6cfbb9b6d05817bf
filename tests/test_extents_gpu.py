"""GPU tier of the band kernels' extents ("past one run, one launch and 4 GiB"): what dg_reduce<>,
dg_observe_rgb<>, dg_plane_nearest<>, dg_observe_distance_nearest<>, the two point kernels, dg_seen_lines<> and their launchers do
past the first of everything.  The other
GPU tiers (tests/test_reduce_gpu.py, tests/test_plane_reduce_gpu.py, tests/test_observe_gpu.py, tests/test_explored_gpu.py) stay at
rows of one run, at most 65 frames and buffers of megabytes.

  runs     every shape of tests/extent_cases.py's table (rows of 2 to 13 runs, short and one-pixel last runs, runs that start off a
           16-byte boundary, short last boxes and bands, both forms of every kernel, 16384 columns, 16384 rows) under every box size of
           np_reduce.FACTORS: dg_reduce_device RGB24 and GRAY8; dg_reduce_planes_device NEAREST and POINT, four planes, per-frame tracer
           planes; dg_observe_device every kind x dtype x layout
  slot     a 2720 x 3 bundle slot: dg_readback_reduced and dg_readback_planes_reduced against the models over the slot's full readbacks
  chunks   65535 (one launch: the control), 65536, 131070 and 131071 frames of a few pixels, random per frame, through the four entry
           points and both forms of each kernel; the kernel-time getter after each call
  big      sources past 2^32 bytes (about 4 060 frames of 1 MB tiled from 3, 16 x 16 boxes) through the four entry points;
           destinations past 2^32 bytes (1 x 1 boxes: the output is the source; a frame stride past 2^32 elements, and one past 2^32 bytes
           only, into observation tensors).  A case whose allocation fails for lack of memory skips with that reason.

Torch tensors are handed to the library in ONE child process (tests/extents/torch_cases.py), because torch has to be imported before
libdoomgpu.so is loaded and this session loaded it long ago; the tests here read the child's per-case results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extent_cases as ec
import np_observe as npo
import np_plane_reduce as npp
import np_reduce as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_IDS = [ec.shape_id(s) for s in ec.SHAPES]
KIND_IDS = [f"source{s}rule{r}" for s, r in npo.KINDS]
CHILD_SECONDS = 120                     # the child's time limit: it takes 16 s on an MI355X, 7 s of them in its 154 cases


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/extents/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("extents") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "extents", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=CHILD_SECONDS)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


def ok_or_out_of_memory(result):
    if result.startswith("out of memory"):
        pytest.skip(result[:300])
    assert result == "ok"


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_reduce_device_past_the_first_run(torch_cases, shape):
    assert torch_cases[f"runs/reduce/{shape}"] == "ok"


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_reduce_planes_device_past_the_first_run(torch_cases, shape):
    assert torch_cases[f"runs/planes/{shape}"] == "ok"


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_observe_device_past_the_first_run(torch_cases, shape, kind):
    assert torch_cases[f"runs/observe/{shape}/{kind}"] == "ok"


def test_reduced_readbacks_of_a_slot_wider_than_one_run(dg, wad1993, path1993):
    """A 2720 x 3 bundle (two full colour runs under fx = 1, second runs off a 16-byte boundary under fx = 3 and 7, two column runs):
    the reduced readbacks against the models over the slot's own full readbacks.  Three rows: the context takes one, but then no box
    size above 1 has a full band."""
    W, H, n = 2720, 3, 3
    scene = dg.Scene(wad1993, "e1m1")
    c = dg.Context(W, H, max_batch=4 * n, slots=1)                            # (a bundle's planes take the room of frames: dg_bundle_capacity)
    assert c.bundle_capacity(7) >= n
    c.upload_scene(scene)
    c.submit_bundle(0, dg.make_views(path1993[[100, 500, 728]]), 7)
    frames = c.readback(0, 0, n).copy()
    planes = dict(zip(npp.NAMES, tuple(c.readback_depth(0, 0, n)) + tuple(c.readback_labels(0, 0, n))[:2]))
    assert frames.any() and len({f.tobytes() for f in frames}) == n and (planes["distance"] != 32767).any()
    for (fx, fy) in ((1, 1), (3, 3), (7, 3), (2, 2), (16, 16)):
        assert len(ec.launch_plan("colour", W, fx)["runs"]) >= 2 and len(ec.launch_plan("column", W, fx)["runs"]) >= 2
        for fmt in (npr.RGB24, npr.GRAY8):
            assert np.array_equal(c.readback_reduced(0, 0, n, (fx, fy, fmt)), npr.reduce(frames, fx, fy, fmt)), (fx, fy, fmt)
        for rule in (npp.POINT, npp.NEAREST):
            got, want = c.readback_planes_reduced(0, 0, n, (fx, fy, rule), boxes=False), npp.reduce(rule, fx, fy, **planes)
            assert set(got) == set(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (fx, fy, rule, k)
    assert np.array_equal(c.readback(0, 0, n), frames)
    c.close()
    scene.close()


@pytest.mark.parametrize("form", ("16", "any"))
@pytest.mark.parametrize("n", ec.FRAME_COUNTS)
@pytest.mark.parametrize("entry", ("reduce", "planes", "observe_rgb", "observe_distance", "seen"))
def test_more_frames_than_one_launch(torch_cases, entry, n, form):
    assert torch_cases[f"chunks/{entry}/{n}/{form}"] == "ok"


@pytest.mark.parametrize("entry", ("reduce", "planes_nearest", "planes_point", "observe_rgb", "observe_nearest", "observe_point", "seen"))
def test_sources_past_2_to_the_32_bytes(torch_cases, entry):
    ok_or_out_of_memory(torch_cases[f"big/source/{entry}"])


@pytest.mark.parametrize("entry", ("reduce", "planes_nearest", "planes_point", "observe_u8_stride", "observe_f32_bytes"))
def test_destinations_past_2_to_the_32_bytes(torch_cases, entry):
    ok_or_out_of_memory(torch_cases[f"big/destination/{entry}"])
