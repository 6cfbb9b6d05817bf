"""CPU tier code-object checks of the observation kernels (observe_kernels.hip): no scratch, no more LDS than the
kernels whose first phase they share; and those kernels (reduce_kernels.hip, plane_reduce_kernels.hip), which now take that phase from
reduce_band.h, keep the LDS, scratch and VGPR numbers they had before it moved."""
from test_wall_fx_isa import _kernels

# (LDS bytes, scratch bytes, VGPRs) with the phase stated inside each kernel, as recorded in DESIGN.md section 8o
PARENT = {
    "dg_reduceILb1E": (12272, 0, 49),
    "dg_reduceILb0E": (12272, 0, 52),
    "dg_plane_nearestILb1E": (8192, 0, 34),
    "dg_plane_nearestILb0E": (8192, 0, 34),
    "dg_plane_point": (0, 0, 7),
}


def _named(ks, part):
    hits = [(n, v) for n, v in ks.items() if part in n]
    assert len(hits) == 1, (part, list(ks))
    return hits[0][1]


def test_reduce_and_plane_reduce_kernels_keep_their_numbers():
    ks = dict(_kernels("reduce_kernels.hip"), **_kernels("plane_reduce_kernels.hip"))
    assert len(ks) == len(PARENT), list(ks)
    for part, want in PARENT.items():
        assert _named(ks, part) == want, part


def test_observe_kernels_have_no_scratch_and_no_more_lds():
    ks = _kernels("observe_kernels.hip")
    assert len(ks) == 5, list(ks)
    lds_max = {"dg_observe_rgbILb1E": PARENT["dg_reduceILb1E"][0], "dg_observe_rgbILb0E": PARENT["dg_reduceILb0E"][0],
               "dg_observe_distance_nearestILb1E": PARENT["dg_plane_nearestILb1E"][0], "dg_observe_distance_nearestILb0E": PARENT["dg_plane_nearestILb0E"][0],
               "dg_observe_distance_point": 0}
    for part, most in lds_max.items():
        lds, scratch, vgpr = _named(ks, part)
        assert scratch == 0 and lds <= most and vgpr <= 64, (part, lds, scratch, vgpr)
