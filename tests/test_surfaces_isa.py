"""CPU tier ISA checks of the per-view surfaces: the surface-reading variants of the device seg walk
(fs_surf_kernels.hip) keep the budgets test_isa_checks.py / test_wall_fx_isa.py hold the existing pairs to (segs: no LDS, <= 16 B
scratch; frame: <= 40.5 KB LDS for four workgroups per CU, <= 160 B scratch; both <= 128 VGPRs), the two flat row kernels
(view_rows_kernels.hip) use no LDS and no scratch, the new frame kernels run fs_frame.h's one phase sequence, and the files that
existed before are not touched by the new policy."""
import os
import re

from test_isa_checks import CSRC
from test_sector_heights_isa import VIEW_ROW_KERNELS, view_row_kernels
from test_wall_fx_isa import _body, _calls, _kernels


def test_surface_reading_pairs_keep_the_seg_walk_budgets():
    ks = _kernels("fs_surf_kernels.hip")
    want = {"dg_sfc_segs": (0, 16), "dg_sfc_frame": (40 * 1024 + 512, 160), "dg_sfc_wfx_segs": (0, 16), "dg_sfc_wfx_frame": (40 * 1024 + 512, 160)}
    assert len(ks) == 4, list(ks)
    for kernel, (lds_max, scratch_max) in want.items():
        hits = [(n, v) for n, v in ks.items() if re.search(rf"\d{kernel}E", n)]
        assert len(hits) == 1, (kernel, list(ks))
        name, (lds, scratch, vgpr) = hits[0]
        assert lds <= lds_max and scratch <= scratch_max and vgpr <= 128, (name, lds, scratch, vgpr)
    assert not any(n in k for k in ks for n in ("dg_fs_segs", "dg_fs_frame", "dg_wfx_segs", "dg_wfx_frame", "dg_hts_"))


def test_flat_row_kernels_use_no_lds_and_no_scratch():
    ks = view_row_kernels()
    for kernel in ("dg_flat_row_fill", "dg_flat_row_scatter"):
        lds, scratch, vgpr = ks[kernel]
        assert lds == 0 and scratch == 0 and vgpr <= VIEW_ROW_KERNELS[kernel], (kernel, lds, scratch, vgpr)


def test_surface_reading_frame_kernels_run_the_one_phase_sequence():
    path = os.path.join(CSRC, "fs_surf_kernels.hip")
    for function in ("dg_sfc_frame", "dg_sfc_wfx_frame"):
        body = _body(path, function)
        assert [c for c in _calls(body) if c != "fs_seg_lane"] == ["FS_FRAME_PHASES"], (function, _calls(body))
        assert "__syncthreads" not in body, function
    for function in ("dg_sfc_segs", "dg_sfc_wfx_segs"):
        assert _calls(_body(path, function)) == ["fs_seg_lane"], function
    assert re.findall(r"\bfs_ph_[a-z_]+\(", open(path).read()) == []


def test_the_default_surfaces_policy_reads_the_scene_tables():
    """Every existing caller of fs_seg names no surfaces policy and so gets FsOwnSurfaces: the emulator and the three existing kernel
    files are untouched by it, and the kernel counts of the files that hold the row-reading pairs and the height row kernels stand."""
    for name in ("fs_kernels.hip", "fs_fx_kernels.hip", "fs_rows_kernels.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "Surfaces" not in txt and "FsSurf" not in txt and "surface_rows" not in txt and "view_rows" not in txt, name
    assert len(_kernels("fs_rows_kernels.hip")) == 4 and len(view_row_kernels()) == 6
    core = open(os.path.join(CSRC, "fs_core.h")).read()
    assert "typename Ht = FsOwnHeights" in core and "const Ht &ht = Ht()" in core
    assert "typename Sf = FsOwnSurfaces" in core and "const Sf &sf = Sf()" in core
    emul = open(os.path.join(os.path.dirname(CSRC), "..", "tests", "emul", "emul.cpp")).read()
    assert "Surfaces" not in emul


def test_section_8p_carries_the_table_of_the_existing_kernels():
    """DESIGN.md section 8p states LDS / scratch / VGPRs of the eight existing seg-walk kernels at the parent and at this commit; the
    second column is what the compiler gives now."""
    design = open(os.path.join(os.path.dirname(CSRC), "..", "DESIGN.md")).read()
    sec = design[design.index("## 8p."):]
    now = {}
    for src in ("fs_kernels.hip", "fs_fx_kernels.hip", "fs_rows_kernels.hip"):
        now.update(_kernels(src))
    assert len(now) == 8
    for kernel in ("dg_fs_segs", "dg_fs_frame", "dg_wfx_segs", "dg_wfx_frame", "dg_hts_segs", "dg_hts_frame", "dg_hts_wfx_segs", "dg_hts_wfx_frame"):
        (lds, scratch, vgpr), = [v for n, v in now.items() if re.search(rf"\d{kernel}E", n)]
        row = re.search(rf"\| `{kernel}` \| (\d+) / (\d+) / (\d+) \| (\d+) / (\d+) / (\d+) \|", sec)
        assert row, kernel
        assert tuple(int(g) for g in row.groups()[3:]) == (lds, scratch, vgpr), (kernel, row.groups(), (lds, scratch, vgpr))
