"""CPU tier ISA checks of the line-of-sight kernels (sight_kernels.hip): no scratch — the pending far children of
a lane's traversal lie in LDS — and exactly the LDS the source declares: SIGHT_MAX_DEPTH 16-bit entries for each of a workgroup's
SIGHT_BLOCK lanes.  The VGPR counts and the waves per SIMD they and the LDS leave are printed for the design note: a record, not a
threshold."""
import os
import re

from test_isa_checks import CSRC
from test_wall_fx_isa import _kernels


def _constant(header, name):
    txt = open(os.path.join(CSRC, header)).read()
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", txt).group(1))


def test_sight_kernels_use_no_scratch_and_the_lds_the_source_declares():
    depth, block = _constant("sight_core.h", "SIGHT_MAX_DEPTH"), _constant("sight_kernels.hpp", "SIGHT_BLOCK")
    declared = depth * block * 2                                # int16_t stacks[SIGHT_MAX_DEPTH * SIGHT_BLOCK]
    ks = _kernels("sight_kernels.hip")
    for kernel in ("dg_sight_queries", "dg_sight_mobjs"):
        hits = [(n, v) for n, v in ks.items() if kernel in n]
        assert len(hits) == 1, (kernel, list(ks))
        name, (lds, scratch, vgpr) = hits[0]
        assert scratch == 0 and lds == declared, (name, lds, scratch)
        alloc = -(-vgpr // 8) * 8                               # the allocation granule is 8 registers per lane
        by_vgpr, by_lds = min(8, 512 // alloc), (160 * 1024 // lds) * (block // 64) // 4
        print(f"{kernel}: {vgpr} VGPRs, {lds} B LDS per {block}-lane workgroup, scratch {scratch}; waves per SIMD: {by_vgpr} by registers, {by_lds} by LDS")
    assert len(ks) == 2, list(ks)
