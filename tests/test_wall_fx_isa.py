"""CPU tier ISA checks of the wall-effect variants of the device seg walk (fs_fx_kernels.hip): the budgets test_isa_checks.py holds
dg_fs_segs and dg_fs_frame to (segs: no LDS, <= 16 B scratch; frame: <= 40.5 KB LDS for four workgroups per CU, <= 160 B scratch; both
<= 128 VGPRs), and both frame kernels and the CPU harness run fs_frame.h's one phase sequence."""
import os
import re
import subprocess

from test_isa_checks import CSRC, FLAGS, HIPCC


def _kernels(src):
    asm = subprocess.run([HIPCC, *FLAGS, "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, src)], capture_output=True, text=True, check=True).stdout
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        body = m.group(2)
        out[m.group(1)] = tuple(int(re.search(rf"\.amdhsa_{k} (\d+)", body).group(1))
                                for k in ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr"))
    return out


def test_wall_fx_kernels_keep_the_seg_walk_budgets():
    ks = _kernels("fs_fx_kernels.hip")
    want = {"dg_wfx_segs": (0, 16), "dg_wfx_frame": (40 * 1024 + 512, 160)}
    for kernel, (lds_max, scratch_max) in want.items():
        hits = [(n, v) for n, v in ks.items() if kernel in n]
        assert len(hits) == 1, (kernel, list(ks))
        name, (lds, scratch, vgpr) = hits[0]
        assert lds <= lds_max and scratch <= scratch_max and vgpr <= 128, (name, lds, scratch, vgpr)
    assert not any("dg_fs_segs" in n or "dg_fs_frame" in n for n in ks)      # (test_isa_checks counts those names in fs_kernels.hip)


def _body(path, function):
    txt = open(path).read()
    body = txt[txt.index(f" {function}("):]
    return body[:body.index("\n}\n")]


def _calls(body):
    return re.findall(r"\b(fs_ph_\w+|fs_seg_lane|FS_FRAME_PHASES)\(", body)


def test_frame_bodies_run_the_one_phase_sequence():
    """fs_frame.h states the phases and their barriers once (FS_FRAME_PHASES); the two frame kernels and the CPU harness each expand it
    once and call no phase themselves, so none of the three can run another order.  The seg kernels are fs_seg_lane and nothing else."""
    emul = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul", "emul.cpp")
    for path, function in ((os.path.join(CSRC, "fs_kernels.hip"), "dg_fs_frame"), (os.path.join(CSRC, "fs_fx_kernels.hip"), "dg_wfx_frame"),
                           (emul, "emul_fs_frame")):
        body = _body(path, function)
        assert [c for c in _calls(body) if c != "fs_seg_lane"] == ["FS_FRAME_PHASES"], (function, _calls(body))
        assert "__syncthreads" not in body, function
    assert _calls(_body(os.path.join(CSRC, "fs_kernels.hip"), "dg_fs_segs")) == ["fs_seg_lane"]
    assert _calls(_body(os.path.join(CSRC, "fs_fx_kernels.hip"), "dg_wfx_segs")) == ["fs_seg_lane"]
    # outside fs_frame.h nothing else names a phase, but the sub-sequence emul_fs_kept_counts runs on purpose
    others = [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC)) if n != "fs_frame.h"] + [emul]
    named = {p: re.findall(r"\bfs_ph_[a-z_]+\(", open(p).read()) for p in others}
    assert {p: v for p, v in named.items() if v} == {emul: ["fs_ph_kept_count(", "fs_ph_block_sums(", "fs_ph_kept_place("]}
    assert re.findall(r"\bfs_ph_[a-z_]+\(", _body(emul, "emul_fs_kept_counts")) == named[emul]
