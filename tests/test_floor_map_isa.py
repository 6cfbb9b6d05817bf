"""CPU tier code-object checks of the floor-textured map frames' kernel (csrc/floor_map_kernels.hip), compiled with
the Makefile's flags: dg_floor_map_tiles has no scratch, the LDS of dg_ego_tiles (the same tile, list and counters), and a VGPR count that
allows at least the waves per SIMD dg_ego_tiles' allows — form by form (tile size x store form), both read from the code objects'
metadata.  A gfx950 SIMD holds 512 VGPRs per lane, handed out in blocks of 8, and at most 8 waves."""
from test_wall_fx_isa import _kernels


def _waves(vgpr: int) -> int:
    return min(8, 512 // (-(-vgpr // 8) * 8))


def _forms(ks, kernel):
    """{(tile words, pixels per item): (lds, scratch, vgpr)} of the kernel template's six instances."""
    out = {}
    for tile in (8192, 16384):
        for px in (16, 4, 1):
            hits = [v for n, v in ks.items() if f"{kernel}ILj{tile}ELi{px}E" in n]
            assert len(hits) == 1, (kernel, tile, px, list(ks))
            out[(tile, px)] = hits[0]
    return out


def test_the_floor_map_kernel_has_no_scratch_and_the_waves_of_the_ego_kernel():
    floor, ego = _forms(_kernels("floor_map_kernels.hip"), "dg_floor_map_tiles"), _forms(_kernels("ego_kernels.hip"), "dg_ego_tiles")
    for form, (lds, scratch, vgpr) in floor.items():
        e_lds, e_scratch, e_vgpr = ego[form]
        print(form, "floor", (lds, scratch, vgpr), "ego", (e_lds, e_scratch, e_vgpr))
        assert scratch == 0 and e_scratch == 0, (form, scratch, e_scratch)
        assert lds == e_lds, (form, lds, e_lds)
        assert _waves(vgpr) >= _waves(e_vgpr), (form, vgpr, e_vgpr)


def test_the_sector_row_kernel_is_small():
    ks = _kernels("floor_map_kernels.hip")
    (lds, scratch, vgpr), = [v for n, v in ks.items() if "dg_floor_seen_sectors" in n]
    assert lds == 0 and scratch == 0 and vgpr <= 16, (lds, scratch, vgpr)
    assert len(ks) == 7, list(ks)
