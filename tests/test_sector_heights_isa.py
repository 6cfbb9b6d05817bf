"""CPU tier ISA checks of the per-view sector heights: the row-reading variants of the device seg walk
(fs_rows_kernels.hip) keep the budgets test_isa_checks.py / test_wall_fx_isa.py hold the existing pairs to (segs: no LDS, <= 16 B
scratch; frame: <= 40.5 KB LDS for four workgroups per CU, <= 160 B scratch; both <= 128 VGPRs), the row kernels of all three kinds
(view_rows_kernels.hip) use no LDS and no scratch, and the new frame kernels run fs_frame.h's one phase sequence."""
import functools
import os
import re

from test_isa_checks import CSRC
from test_wall_fx_isa import _body, _calls, _kernels


def test_row_reading_pairs_keep_the_seg_walk_budgets():
    ks = _kernels("fs_rows_kernels.hip")
    want = {"dg_hts_segs": (0, 16), "dg_hts_frame": (40 * 1024 + 512, 160), "dg_hts_wfx_segs": (0, 16), "dg_hts_wfx_frame": (40 * 1024 + 512, 160)}
    assert len(ks) == 4, list(ks)
    for kernel, (lds_max, scratch_max) in want.items():
        hits = [(n, v) for n, v in ks.items() if kernel in n]
        assert len(hits) == 1, (kernel, list(ks))
        name, (lds, scratch, vgpr) = hits[0]
        assert lds <= lds_max and scratch <= scratch_max and vgpr <= 128, (name, lds, scratch, vgpr)
    assert not any(n in k for k in ks for n in ("dg_fs_segs", "dg_fs_frame", "dg_wfx_segs", "dg_wfx_frame"))


# The six row kernels of view_rows_kernels.hip and their VGPR bounds: 32 for the sector and flat kernels as ever; for the two pose
# kernels the 6 and 14 they had as a translation unit of their own.
VIEW_ROW_KERNELS = {"dg_mobj_pose_fill": 6, "dg_mobj_pose_place": 14, "dg_sector_row_fill": 32, "dg_sector_row_scatter": 32,
                    "dg_flat_row_fill": 32, "dg_flat_row_scatter": 32}


@functools.lru_cache(maxsize=None)
def view_row_kernels():
    """name -> (lds, scratch, vgpr) of the six, each found exactly once among exactly six (compiled once for the tests that ask)."""
    ks = _kernels("view_rows_kernels.hip")
    assert len(ks) == 6, list(ks)
    out = {}
    for kernel in VIEW_ROW_KERNELS:
        hits = [v for n, v in ks.items() if re.search(rf"\d{kernel}E", n)]
        assert len(hits) == 1, (kernel, list(ks))
        out[kernel] = hits[0]
    return out


def test_row_kernels_use_no_lds_and_no_scratch():
    ks = view_row_kernels()
    for kernel in ("dg_sector_row_fill", "dg_sector_row_scatter", "dg_mobj_pose_fill", "dg_mobj_pose_place"):
        lds, scratch, vgpr = ks[kernel]
        assert lds == 0 and scratch == 0 and vgpr <= VIEW_ROW_KERNELS[kernel], (kernel, lds, scratch, vgpr)


def test_row_reading_frame_kernels_run_the_one_phase_sequence():
    path = os.path.join(CSRC, "fs_rows_kernels.hip")
    for function in ("dg_hts_frame", "dg_hts_wfx_frame"):
        body = _body(path, function)
        assert [c for c in _calls(body) if c != "fs_seg_lane"] == ["FS_FRAME_PHASES"], (function, _calls(body))
        assert "__syncthreads" not in body, function
    for function in ("dg_hts_segs", "dg_hts_wfx_segs"):
        assert _calls(_body(path, function)) == ["fs_seg_lane"], function
    assert re.findall(r"\bfs_ph_[a-z_]+\(", open(path).read()) == []


def test_the_default_heights_policy_reads_the_scene_table():
    """Every existing caller of fs_seg / fs_mobj names no heights policy and so gets FsOwnHeights: the emulator and the two existing kernel
    files are untouched by the rows."""
    for name in ("fs_kernels.hip", "fs_fx_kernels.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "FsRowHeights" not in txt and "FsWithRows" not in txt and "sector_rows" not in txt and "view_rows" not in txt, name
    core = open(os.path.join(CSRC, "fs_core.h")).read()
    assert "typename Ht = FsOwnHeights" in core and "const Ht &ht = Ht()" in core
