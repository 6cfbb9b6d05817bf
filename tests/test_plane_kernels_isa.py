"""CPU tier resource budgets of the plane walk's kernels (csrc/plane_kernels.hip), compiled with the Makefile's flags: the six kernels
that must be there, the staging each keeps in LDS (16 spans x 8 or 9 words x 64 columns: four workgroups per CU), no scratch, and the
VGPRs each separate kernel had before the three were made one body — none above 64, so all keep 8 waves per SIMD."""
from test_wall_fx_isa import _kernels

#          kernel                                LDS bytes        VGPR ceiling
BUDGETS = {"dg_depth_tiles":                     (32768, "==", 58),
           "dg_label_tiles":                     (32768, "==", 54),
           "dg_label_boxes":                     (0,     "==", 14),
           "dg_bundle_tilesILb1ELb1EE":          (36864, "==", 64),      # z and the owner tag: the ninth word
           "dg_bundle_tilesILb1ELb0EE":          (32768, "==", 58),
           "dg_bundle_tilesILb0ELb1EE":          (36864, "<=", 63)}      # (the tag in word 3: no ninth word)


def test_the_plane_kernels_keep_their_lds_scratch_and_vgpr_budgets():
    ks = _kernels("plane_kernels.hip")
    assert len(ks) == len(BUDGETS), list(ks)
    for kernel, (lds_want, rel, vgpr_max) in BUDGETS.items():
        hits = [(n, v) for n, v in ks.items() if kernel in n]
        assert len(hits) == 1, (kernel, list(ks))
        name, (lds, scratch, vgpr) = hits[0]
        print(name, "lds", lds, "scratch", scratch, "vgpr", vgpr)
        assert (lds == lds_want if rel == "==" else lds <= lds_want) and scratch == 0 and vgpr <= vgpr_max, (name, lds, scratch, vgpr)
