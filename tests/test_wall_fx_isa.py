"""CPU tier ISA checks of the wall-effect variants of the device seg walk (fs_fx_kernels.hip): the budgets test_isa_checks.py holds
dg_fs_segs and dg_fs_frame to (segs: no LDS, <= 16 B scratch; frame: <= 40.5 KB LDS for four workgroups per CU, <= 160 B scratch; both
<= 128 VGPRs), and dg_wfx_frame runs dg_fs_frame's phases in the same order."""
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


def _phases(src, kernel):
    txt = open(os.path.join(CSRC, src)).read()
    body = txt[txt.index(f"void {kernel}("):]
    body = body[:body.index("\n}\n")]
    return re.findall(r"\b(fs_ph_\w+|fs_seg_lane|__syncthreads)\(", body)


def test_wall_fx_frame_runs_the_same_phases():
    assert _phases("fs_fx_kernels.hip", "dg_wfx_frame") == _phases("fs_kernels.hip", "dg_fs_frame")
    assert _phases("fs_fx_kernels.hip", "dg_wfx_segs") == _phases("fs_kernels.hip", "dg_fs_segs") == ["fs_seg_lane"]
