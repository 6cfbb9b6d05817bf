"""CPU tier code-object checks of the map frames with map-object markers (csrc/map_things_kernels.hip), compiled with
the Makefile's flags: the twelve instances of dg_ego_thing_tiles and dg_floor_thing_tiles have no scratch and the LDS of dg_ego_tiles
(the same tile, list and counters: the things phase adds none) — form by form (tile size x store form), read from the code objects'
metadata.  The unit holds these twelve kernels and nothing else, and the two plain units keep theirs."""
from test_floor_map_isa import _forms
from test_wall_fx_isa import _kernels


def test_the_twelve_thing_kernels_have_no_scratch_and_the_lds_of_the_ego_kernel():
    ks = _kernels("map_things_kernels.hip")
    ego = _forms(_kernels("ego_kernels.hip"), "dg_ego_tiles")
    assert len(ks) == 12, list(ks)
    for kernel in ("dg_ego_thing_tiles", "dg_floor_thing_tiles"):
        for form, (lds, scratch, vgpr) in _forms(ks, kernel).items():
            e_lds, e_scratch, _ = ego[form]
            print(kernel, form, (lds, scratch, vgpr), "ego", ego[form])
            assert scratch == 0 and e_scratch == 0, (kernel, form, scratch)
            assert lds == e_lds, (kernel, form, lds, e_lds)


def test_the_plain_units_keep_their_kernels():
    assert len(_kernels("ego_kernels.hip")) == 6 and len(_kernels("floor_map_kernels.hip")) == 7
