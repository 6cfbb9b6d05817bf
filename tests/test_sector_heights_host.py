"""Per-view sector heights on the CPU (include/doomgpu.h: dg_view_sectors): the host walker with sector entries
and the host-only calls.  Everything is byte-exact.

  oracle          dg_build_lists_sectors of the UNPATCHED scene -> the emulator's list rasteriser equals the oracle's frame of the WAD
                  whose SECTORS records were patched to the same heights (tests/sector_height_cases.py): the named cases on sectors
                  the view sees, and 60 dense random rows in four modes, on three maps
  planes          the same cases through dg_depth_lists_host / dg_label_lists_host / dg_bundle_lists_host against lists built from the
                  product's own scene of the patched WAD
  composition     with light / state entries and the wall, light and map-object effects on
  errors          every error return of the new host calls; NULL and n = 0 give the bytes of the existing calls
  stand-alone     tests/sector_heights/sector_heights_host_main.cpp under AddressSanitizer + UBSan, as a program
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emul_bind
import mobj_fx as mf
import mobj_pose_cases as mp
import sector_height_cases as sh
from conftest import ROOT, load_path

W, H = sh.W, sh.H
MAPS = [(1993, False), (1994, False), (1995, True)]
NAMES = ["shut", "half", "inverted", "lift", "raise", "floor_over", "floor_min", "ceil_max", "own", "sky", "all", "same", "duplicates", "rides"]


def _lists_bytes(dg, fl):
    return (ctypes.string_at(fl.renders, fl.n_renders * ctypes.sizeof(dg.DgBitmapRender)), ctypes.string_at(fl.columns, fl.n_columns * ctypes.sizeof(dg.DgBitmapColumn)),
            ctypes.string_at(fl.visplanes, fl.n_visplanes * ctypes.sizeof(dg.DgVisplane)), ctypes.string_at(fl.plane_tb, fl.n_plane_tb * 2),
            ctypes.string_at(fl.order, fl.n_order * ctypes.sizeof(dg.DgDrawCmd)))


@pytest.fixture(scope="module", params=MAPS, ids=lambda p: f"seed{p[0]}")
def world(request, dg, synth, oracle, wad1993, wad1994, wad1995):
    seed, _ = request.param
    wad = {1993: wad1993, 1994: wad1994, 1995: wad1995}[seed]
    scene = dg.Scene(wad, "e1m1")
    path = load_path(seed)
    out = {"seed": seed, "wad": wad, "scene": scene, "path": path, "emul": emul_bind.EmulScene(wad)}
    pairs = sh.visible_pairs(oracle, wad, path)              # (every sector of 26 frames: the search is the fixture's cost)
    out["pairs"] = pairs
    out["sky_pair"] = sh.find_sky_pair(oracle, wad, path, pairs)
    out["cases"] = sh.named_cases(scene, oracle, wad, path, pairs, out["sky_pair"])
    return out


def _view(dg, case, path):
    return dg.make_views(case.record(path)[None])[0]


def _product_frame(dg, world, case):
    fl = world["scene"].build_lists_sectors(W, H, _view(dg, case, world["path"]), [tuple(e) for e in case.entries], mp.entries_as_poses(case.poses) if case.poses else None)
    return np.frombuffer(world["emul"].draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)


def _assert_same(got, want, what):
    bad = np.argwhere(np.any(got != want, axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ from the oracle, first at (x={bad[0][1]}, y={bad[0][0]})"


def test_scene_sector_heights_equal_the_lump(world):
    got = world["scene"].sector_heights()
    assert got.dtype == np.int16 and np.array_equal(got, sh.loaded_heights(world["wad"])) and len(got) == world["scene"].sector_count()
    assert len(got) == {1993: 105, 1994: 435, 1995: 108}[world["seed"]]


def test_a_sky_ceilinged_sector_is_visible_on_one_of_the_maps(dg, oracle, wad1993, wad1995, path1993, path1995):
    found = [sh.find_sky_pair(oracle, w, p, sh.visible_pairs(oracle, w, p)) for w, p in ((wad1993, path1993), (wad1995, path1995))]
    assert any(f is not None for f in found), "no visible sky-ceilinged sector on seed 1993 or 1995"


def test_named_cases_equal_the_oracle_of_the_patched_wad(dg, oracle, world):
    wad, path = world["wad"], world["path"]
    names = [c.name for c in world["cases"]]
    assert names == [n for n in NAMES if n != "sky" or world["sky_pair"] is not None], names
    assert len(world["pairs"]) >= 20
    for c in world["cases"]:
        want = sh.oracle_frame(oracle, c.patched(wad), c.record(path), W, H)
        _assert_same(_product_frame(dg, world, c), want, c)
        base = mp.patch_things(wad, mp.resolved(c.poses)) if c.poses else wad
        plain = sh.oracle_frame(oracle, base, path[c.frame], W, H)     # (rides: the same pose with the floor unmoved)
        assert np.array_equal(want, plain) != c.changes, c


def test_sixty_dense_random_rows_equal_the_oracle(dg, oracle, world):
    wad, path = world["wad"], world["path"]
    for c in sh.random_cases(wad, 60, seed=world["seed"]):
        want = sh.oracle_frame(oracle, c.patched(wad), c.record(path), W, H)
        _assert_same(_product_frame(dg, world, c), want, c)
        if c.name.startswith(("jitter", "random")):          # (these two modes move every sector, the ones in view among them)
            assert not np.array_equal(want, sh.oracle_frame(oracle, wad, path[c.frame], W, H)), c


def test_planes_equal_those_of_the_scene_of_the_patched_wad(dg, world):
    """Depth, label and bundle planes of lists built with entries on the unpatched scene equal those of the product's own scene of the
    patched WAD; so do the lists and owner tags themselves."""
    wad, scene, path = world["wad"], world["scene"], world["path"]
    cases = world["cases"] + sh.random_cases(wad, 8, seed=7 + world["seed"])
    for c in cases:
        view = _view(dg, c, path)
        fl, own = scene.build_lists_sectors(W, H, view, [tuple(e) for e in c.entries], mp.entries_as_poses(c.poses) if c.poses else None, owners=True)
        got_lists = _lists_bytes(dg, fl)
        frames = (dg.DgFrameLists * 1)(fl)
        got = (dg.depth_lists_host(scene, W, H, frames), dg.label_lists_host(scene, W, H, frames, [own]), dg.bundle_lists_host(scene, W, H, frames, [own]))
        patched = dg.Scene(c.patched(wad), "e1m1")
        fl2, own2 = patched.build_lists_owners(W, H, view)
        assert got_lists == _lists_bytes(dg, fl2) and np.array_equal(own, own2), c
        frames2 = (dg.DgFrameLists * 1)(fl2)
        want = (dg.depth_lists_host(patched, W, H, frames2), dg.label_lists_host(patched, W, H, frames2, [own2]), dg.bundle_lists_host(patched, W, H, frames2, [own2]))
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert np.array_equal(a, b), c
        patched.close()


def test_null_and_empty_entries_give_the_bytes_of_the_existing_calls(dg, world):
    scene = world["scene"]
    for f in (217, 640):
        view = dg.make_views(world["path"][[f]])[0]
        plain = _lists_bytes(dg, scene.build_lists(W, H, view))
        assert _lists_bytes(dg, scene.build_lists_sectors(W, H, view, None)) == plain
        assert _lists_bytes(dg, scene.build_lists_sectors(W, H, view, [])) == plain
        assert _lists_bytes(dg, scene.build_lists_poses(W, H, view, None)) == plain
        hs = sh.loaded_heights(world["wad"])
        assert _lists_bytes(dg, scene.build_lists_sectors(W, H, view, [(s, int(hs[s, 0]), int(hs[s, 1])) for s in range(len(hs))])) == plain
        assert len(plain[0]) > 0


def test_composition_with_view_state_and_the_three_effects(dg, oracle, world):
    """Sector entries on top of light / state entries, with the wall, light and map-object effects switched on: the product's scene of the
    patched WAD, set up the same way, builds the same lists; with the light entries alone the oracle agrees as well."""
    wad, scene, path = world["wad"], world["scene"], world["path"]
    n = scene.sector_count()
    cases = [c for c in world["cases"] if c.name in ("shut", "lift", "all", "rides")]
    # light entries: the oracle has a setter for them
    for k, c in enumerate(cases):
        lights = [((k * 11 + j * 7) % n, (j * 53 + 40) % 256) for j in range(9)]

        def prepare(osc):
            for s, level in lights:
                osc.set_sector_light(s, level)
        want = sh.oracle_frame(oracle, c.patched(wad), c.record(path), W, H, prepare=prepare)
        tuned = dg.Scene(wad, "e1m1")
        for s, level in lights:
            tuned.set_sector_light(s, level)
        fl = tuned.build_lists_sectors(W, H, _view(dg, c, path), [tuple(e) for e in c.entries], mp.entries_as_poses(c.poses) if c.poses else None)
        _assert_same(np.frombuffer(world["emul"].draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3), want, c)
        tuned.close()
    # the three effects: the product's scene of the patched WAD with the same effects
    for c in cases:
        a, b = dg.Scene(wad, "e1m1"), dg.Scene(c.patched(wad), "e1m1")
        for sc in (a, b):
            sc.set_wall_effects(dg.DG_WALL_ANIMATE | dg.DG_WALL_SCROLL)
            sc.set_light_effects(dg.DG_LIGHT_THINKERS, 5)
            sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
        rec = np.concatenate([c.record(path), np.float32([3.7])])
        view = dg.make_views(rec[None, :8], timestamp=3.7)[0]
        got = _lists_bytes(dg, a.build_lists_sectors(W, H, view, [tuple(e) for e in c.entries], mp.entries_as_poses(c.poses) if c.poses else None))
        assert got == _lists_bytes(dg, b.build_lists(W, H, view)), c
        a.close(); b.close()


def test_argument_errors(dg, world):
    L, scene = dg.lib(), world["scene"]
    n = scene.sector_count()
    view = dg.make_views(world["path"][[0]])[0]
    fl = dg.DgFrameLists()
    for bad in (n, n + 7, -1, 1 << 20):
        with pytest.raises(dg.DoomGpuError) as e:
            scene.build_lists_sectors(W, H, view, [(0, 0, 128), (bad, 0, 128)])
        assert e.value.code == dg.DG_ERR_INVALID and "sector index out of range" in str(e.value)
    for f, c in ((-32769, 0), (32768, 0), (0, -32769), (0, 32768), (1 << 20, 0)):
        with pytest.raises(dg.DoomGpuError) as e:
            scene.build_lists_sectors(W, H, view, [(0, f, c)])
        assert e.value.code == dg.DG_ERR_INVALID and "height outside int16" in str(e.value)
    scene.build_lists_sectors(W, H, view, [(0, -32768, 32767), (n - 1, 32767, -32768)])
    vs = dg.DgViewSectors(None, 3)
    assert L.dg_build_lists_sectors(scene._h, W, H, ctypes.byref(view), None, ctypes.byref(vs), ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_sectors(None, W, H, ctypes.byref(view), None, None, ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_sectors(scene._h, W, H, None, None, None, ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_sectors(scene._h, W, H, ctypes.byref(view), None, None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_sectors(scene._h, W, H, ctypes.byref(view), None, None, ctypes.byref(fl), None) == dg.DG_OK
    vs0 = dg.DgViewSectors(None, 0)
    assert L.dg_build_lists_sectors(scene._h, W, H, ctypes.byref(view), None, ctypes.byref(vs0), ctypes.byref(fl), None) == dg.DG_OK
    a, b = np.zeros(n + 1, dtype=np.int16), np.zeros(n + 1, dtype=np.int16)
    for bad_n in (n - 1, n + 1, 0, -1):
        assert L.dg_scene_sector_heights(scene._h, a.ctypes.data, b.ctypes.data, bad_n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_heights(None, a.ctypes.data, b.ctypes.data, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_heights(scene._h, None, b.ctypes.data, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_heights(scene._h, a.ctypes.data, None, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_sector_heights(scene._h, a.ctypes.data, b.ctypes.data, n) == dg.DG_OK
    assert (ctypes.sizeof(dg.DgSectorHeights), ctypes.sizeof(dg.DgViewSectors)) == (12, 16) and b"ABI 4" in L.dg_version()


def test_the_binding_and_the_header_carry_the_sector_height_entry_points(dg):
    declared = dg.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", dg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in ("dg_submit_views_sectors", "dg_render_views_sectors", "dg_submit_bundle_views_sectors", "dg_build_lists_sectors", "dg_scene_sector_heights",
              "dg_slot_sector_heights", "dg_slot_sector_height_timing"):
        assert n in declared and n in exported and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    for n in ("submit_sectors", "render_sectors", "submit_bundle_sectors", "slot_sector_heights", "sector_height_timing"):
        assert callable(getattr(dg.Context, n)), n
    assert callable(dg.make_view_sectors) and callable(dg.Scene.sector_heights) and callable(dg.Scene.build_lists_sectors)


def test_the_row_bodies_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/sector_heights/sector_heights_host_main.cpp (its own main) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: resolve_view_sectors, LatestPerIndex, view_rows_core.h's fill and scatter bodies lane after lane
    at the kernels' boundary counts, then build_frame_lists with entries.  It checks its own results; any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "sector_heights_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "sector_heights", "sector_heights_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "light.wad"
    wad.write_bytes(wad1993)
    r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "sector_heights_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
