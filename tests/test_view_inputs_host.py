"""A view's four optional inputs on the host (csrc/frontend.hpp: ViewInputs, BatchInputs, KeptInputs, check_view_inputs; DESIGN.md
section 8r), without a GPU: the slot's kept copy, the null-array rule and the host walker taking one ViewInputs."""
import os
import subprocess

from conftest import ROOT


def test_the_kept_copy_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/view_inputs/view_inputs_host_main.cpp (its own main) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: KeptInputs::keep over 1, 2 and 5 views with 0, 1 and 7 entries and null arrays,
    the caller's storage overwritten and freed before the copy is read; a second keep; check_view_inputs' four messages;
    build_frame_lists with a ViewInputs against dg_build_lists_surfaces.  It checks its own results; any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "view_inputs_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "view_inputs", "view_inputs_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "inputs.wad"
    wad.write_bytes(wad1993)
    r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "view_inputs_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
