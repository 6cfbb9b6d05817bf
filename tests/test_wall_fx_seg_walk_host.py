"""CPU tier of the device seg walk with the wall effects (dg_wfx_segs / dg_wfx_frame: fs_frame.h's bodies and phase sequence given FsFx):
tests/emul runs them lane by lane on the fixture WAD with the effects on and compares, inside the harness, every record with the host
walker's for the same scene — over test_wall_fx_host's timestamps and views, none excused; and the effects do reach these views."""
import pytest

import emul_bind
import wall_fx as wf
from test_wall_fx_host import GRID, VIEWS

W, H = 320, 200


@pytest.fixture(scope="module")
def wad():
    return wf.fx_wad()


@pytest.mark.parametrize("flags", [wf.ANIMATE, wf.SCROLL, wf.ANIMATE | wf.SCROLL])
def test_device_walk_equals_the_host_walker_with_the_effects(wad, path1993, flags):
    es = emul_bind.EmulScene(wad, "E1M1")
    es.set_wall_effects(flags)
    for t in GRID:
        for i in VIEWS:
            rc, st = es.fs_frame(W, H, path1993[i], t)
            assert rc == 0, (flags, t, i, rc, st, emul_bind.lib().emul_last_error())


def test_the_effects_reach_these_views(wad, path1993):
    plain, es = emul_bind.EmulScene(wad, "E1M1"), emul_bind.EmulScene(wad, "E1M1")
    es.set_wall_effects(wf.ANIMATE | wf.SCROLL)
    changed = sum(es.frame_parts(W, H, path1993[i], 7.3) != plain.frame_parts(W, H, path1993[i], 7.3) for i in VIEWS)
    assert changed >= 3, changed
