"""CPU tier resource budgets of the screen pictures' kernel (csrc/overlay_kernels.hip), compiled with the
Makefile's flags: no scratch, and at most 64 VGPRs, so that it keeps 8 waves per SIMD."""
from test_wall_fx_isa import _kernels


def test_the_overlay_kernel_has_no_scratch_and_at_most_64_vgprs():
    ks = _kernels("overlay_kernels.hip")
    hits = [(n, v) for n, v in ks.items() if "dg_overlay_tiles" in n]
    assert len(hits) == 1 and len(ks) == 1, list(ks)
    name, (lds, scratch, vgpr) = hits[0]
    print(name, "lds", lds, "scratch", scratch, "vgpr", vgpr)
    assert scratch == 0 and vgpr <= 64, (name, lds, scratch, vgpr)
