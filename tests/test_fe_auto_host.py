"""CPU tier of DG_FE_AUTO's policy (csrc/fe_auto.hpp): tests/fe_auto/fe_auto_main.cpp drives the struct alone — nothing in flight, the probe
cadences of 32 and 256 batches in both directions, the host and GPU running means and the first samples they drop — built with the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fe_auto_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fe_auto") / "fe_auto_main"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "fe_auto", "fe_auto_main.cpp"), "-o", str(exe)])
    return str(exe)


def test_auto_policy_decisions_and_means(fe_auto_main):
    r = subprocess.run([fe_auto_main], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    # nothing in flight, the three cadences (cycles x (run + 1) decisions), host samples, calibration, GPU samples: none skipped
    assert int(r.stdout.split()[1]) == 601 + 3 * 32 + (2 * 256 + 2 * 32) + (3 * 32 + 32) + 3 + 5 + 6
