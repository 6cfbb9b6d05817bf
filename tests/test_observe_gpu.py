"""GPU tier of the observation tensors: dg_observe_device into torch tensors, every result bit pattern for bit
pattern against the numpy restatement (np_observe), sentinel elements around and inside every destination included.  All cases run in
ONE child process (tests/observe/torch_cases.py), because torch has to be imported before libdoomgpu.so is loaded and this session
loaded it long ago; the tests here read the child's per-case results.

  grid       np_reduce.SIZES x np_reduce.FACTORS for (RGB, F32, NCHW), 1, 3 and 65 frames (1 and 3 at 320x200)
  combos     every source/rule x dtype x layout at every size of np_reduce.SIZES and four box sizes, the frame counts and maps taking
             turns.  A row of 64, 80 or 320 pixels is a multiple of 16 bytes in both source formats, so these take the 16-byte kernels;
             131x67, 5x9 and 1x1 take the any-width ones; 16x16 on 5x9 and 1x1 is a box larger than the frame.  Every row of this
             file is ONE run of its band kernel (blockIdx.x == 0), every call one launch: rows of several runs, obs_item in a short
             last run, more than 65535 frames and offsets past 2^32 are tests/test_extents_gpu.py's
  unaligned  64x40 sources one byte (colour) or two bytes (distance) off a 16-byte boundary: the any-width kernels at a 16-byte width
  maps       every map of np_observe.MAPS / U8_MAPS on every source and dtype
  sweep      every int16 once through tensors of the four dtypes, by observe_into; observe_into's refusals
  composed   RGB + distance into one RGB-D float16 tensor by two calls; gray into slot t % 4 of a frame stack over 6 steps
  slot       a bundle slot's own colour frames and distance plane as sources; observations with two slots in flight leave the slots'
             frames, planes, timing counts and fallback counters alone; observe_kernel_ms() > 0
  errors     the error returns that need a ctx"""
import json
import os
import subprocess
import sys

import pytest

import np_observe as npo
import np_reduce as npr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_IDS = [f"source{s}rule{r}" for s, r in npo.KINDS]


@pytest.fixture(scope="module")
def torch_cases(tmp_path_factory):
    """What tests/observe/torch_cases.py found, case name -> "ok" or the failure: one child process for all of them."""
    out = tmp_path_factory.mktemp("observe") / "torch_cases.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "observe", "torch_cases.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and out.exists(), f"torch_cases.py ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.load(open(out))


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("factor", npr.FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_rgb_f32_nchw_over_the_reduce_grid(torch_cases, size, factor):
    assert torch_cases[f"grid/{size[0]}x{size[1]}/{factor[0]}x{factor[1]}"] == "ok"


@pytest.mark.parametrize("size", npr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KIND_IDS)
def test_every_source_dtype_and_layout(torch_cases, size, kind):
    assert torch_cases[f"combos/{size[0]}x{size[1]}/{kind}"] == "ok"


@pytest.mark.parametrize("kind", KIND_IDS)
def test_sources_off_the_16_byte_boundary(torch_cases, kind):
    assert torch_cases[f"unaligned/{kind}"] == "ok"


@pytest.mark.parametrize("kind", KIND_IDS)
def test_every_map(torch_cases, kind):
    assert torch_cases[f"maps/{kind}"] == "ok"


def test_the_sweep_of_every_int16_through_observe_into(torch_cases):
    assert torch_cases["sweep"] == "ok"


def test_composed_tensors(torch_cases):
    assert torch_cases["composed"] == "ok"


def test_slot_sources_and_slots_in_flight(torch_cases):
    assert torch_cases["slot"] == "ok"


def test_observe_device_errors(torch_cases):
    assert torch_cases["errors"] == "ok"
