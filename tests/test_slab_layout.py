"""CPU tier of the slab layouts (csrc/slab_layout.h): tests/slab_layout/layout_check.cpp walks a grid of widths, batch sizes, scene sizes
and effect switches and checks alignment, order, non-overlap, monotonicity and that a full batch at its caps fits dg_create's capacity.
The record headers it includes need the library's own two warning exemptions (unused parameters, `#pragma unroll` under g++)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slab_layout") / "layout_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "slab_layout", "layout_check.cpp"), "-o", str(exe)])
    return str(exe)


def test_slab_layouts_hold_over_the_grid(layout_check):
    r = subprocess.run([layout_check], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    configs, checks = (int(v) for v in r.stdout.split()[1:3])
    # 3 widths x 3 batch sizes x (1 + 8 switch settings x 3 scene sizes + 5 seg counts): none skipped
    assert configs == 3 * 3 * (1 + 8 * 3 + 5) and checks > configs
