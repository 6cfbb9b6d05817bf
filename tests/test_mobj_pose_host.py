"""Per-view map-object poses on the CPU (include/doomgpu.h: dg_view_poses): the host walker with poses, the host-only
calls, and the shared fill / scatter bodies of view_rows_core.h for the pose kind (mobj_pose_core.h).  Everything is byte-exact.

  oracle          dg_build_lists_poses -> the emulator's list rasteriser equals the oracle's frame of the WAD whose THINGS records were
                  patched to the same poses (tests/mobj_pose_cases.py): one object, all objects, across a floor step, into another light,
                  a full-bright object, the loaded pose (lists byte for byte dg_build_lists'), duplicate entries
  patched scene   the lists and owner tags equal those of the product's own scene of the patched WAD: the tags keep their indices
  fractional      fractional positions and arbitrary angles against the second renderer (np_front_end.render_frame)
  sectors         dg_scene_sectors_at against np_front_end.get_sector_from_vertex: random points, points on and within an ulp of partition
                  lines, vertices, NaN and infinities, and a map with holes, where an object moved into no sector is not drawn; on the
                  hand world's oblique partition the points at which a fused side test finds the other sector, and exact ties
  errors          every error return of the new host calls
  stand-alone     tests/mobj_pose/mobj_pose_host_main.cpp under AddressSanitizer + UBSan, as a program
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emul_bind
import mobj_pose_cases as mp
import walk_cases
from conftest import ROOT, load_path

W, H = mp.W, mp.H
MAPS = [(1993, False), (1995, True)]


def _lists_bytes(dg, fl):
    """The five arrays of a dg_frame_lists, copied out of the arena."""
    return (ctypes.string_at(fl.renders, fl.n_renders * ctypes.sizeof(dg.DgBitmapRender)), ctypes.string_at(fl.columns, fl.n_columns * ctypes.sizeof(dg.DgBitmapColumn)),
            ctypes.string_at(fl.visplanes, fl.n_visplanes * ctypes.sizeof(dg.DgVisplane)), ctypes.string_at(fl.plane_tb, fl.n_plane_tb * 2),
            ctypes.string_at(fl.order, fl.n_order * ctypes.sizeof(dg.DgDrawCmd)))


@pytest.fixture(scope="module", params=MAPS, ids=lambda p: f"seed{p[0]}")
def world(request, dg, synth, oracle):
    seed, vanilla = request.param
    wad = synth.build_synth_iwad(seed, vanilla=vanilla)
    scene = dg.Scene(wad, "e1m1")
    path = load_path(seed)
    cases = mp.named_cases(scene, wad, path)
    frames = mp.oracle_frames(oracle, wad, path, cases, W, H)
    return {"seed": seed, "wad": wad, "scene": scene, "path": path, "cases": cases, "oracle_frames": frames, "emul": emul_bind.EmulScene(wad)}


def test_the_float_formula_reproduces_the_loader(world):
    mp.assert_formula(world["scene"], world["wad"])
    placed = world["scene"].mobj_poses()
    assert np.array_equal(placed["sector"], world["scene"].sectors_at(placed["x"], placed["y"]))


def test_lists_with_poses_equal_the_oracle_of_the_patched_wad(dg, world):
    scene, path = world["scene"], world["path"]
    names = [c.name for c in world["cases"]]
    assert names == ["one", "all", "floor_step", "other_light", "full_bright", "same", "duplicates"]
    for c, want in zip(world["cases"], world["oracle_frames"]):
        view = dg.make_views(path[[c.frame]])[0]
        fl = scene.build_lists_poses(W, H, view, mp.entries_as_poses(c.entries))
        got = np.frombuffer(world["emul"].draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)
        bad = np.argwhere(np.any(got != want, axis=2))
        assert len(bad) == 0, f"{c}: {len(bad)} pixels differ from the oracle, first at (x={bad[0][1]}, y={bad[0][0]})"


def test_the_loaded_pose_gives_the_lists_of_dg_build_lists(dg, world):
    scene = world["scene"]
    c = next(c for c in world["cases"] if c.name == "same")
    view = dg.make_views(world["path"][[c.frame]])[0]
    with_poses = _lists_bytes(dg, scene.build_lists_poses(W, H, view, mp.entries_as_poses(c.entries)))
    no_entries = _lists_bytes(dg, scene.build_lists_poses(W, H, view, []))
    null_poses = _lists_bytes(dg, scene.build_lists_poses(W, H, view, None))
    plain = _lists_bytes(dg, scene.build_lists(W, H, view))
    assert with_poses == plain and no_entries == plain and null_poses == plain
    assert len(plain[0]) > 0


def test_lists_and_owner_tags_equal_the_scene_of_the_patched_wad(dg, world):
    """What the product's own loader makes of the patched THINGS lump is what a pose makes of the unpatched scene: the same lists, and
    the same owner tags — a moved object keeps its index."""
    scene, path = world["scene"], world["path"]
    moved_seen = 0
    for c in world["cases"]:
        view = dg.make_views(path[[c.frame]])[0]
        fl, own = scene.build_lists_poses(W, H, view, mp.entries_as_poses(c.entries), owners=True)
        got = _lists_bytes(dg, fl)
        patched = dg.Scene(mp.patch_things(world["wad"], mp.resolved(c.entries)), "e1m1")
        fl2, own2 = patched.build_lists_owners(W, H, view)
        assert got == _lists_bytes(dg, fl2), c
        assert np.array_equal(own, own2), c
        patched.close()
        tags = {int(t) & 0xFFFF for t in own if int(t) >> 16 == dg.DG_LABEL_MOBJ}
        moved_seen += len(tags & set(mp.resolved(c.entries)))
    assert moved_seen > 5                                     # moved objects really are among the draw records


def test_fractional_poses_equal_the_second_renderer(dg, world):
    import np_front_end as nf
    import np_mappers as nm
    wad, scene, path = world["wad"], world["scene"], world["path"]
    np_map, np_wad, sprites = nf.Map(wad, "e1m1"), nm.Wad(wad), nf.SpriteTable(wad)
    base = nf.load_things(wad, "e1m1")
    assert len(base) == scene.mobj_count()                    # no S_NULL spawn states on these maps: the two orders are one
    F = np.float32
    changed = 0
    for f in ((100, 431) if world["seed"] == 1993 else (323,)):
        r = path[f]
        entries = []
        for j, m in enumerate((1, 6, 17, 33)):
            t = path[(f + 8 + 5 * j) % 1000]
            entries.append((m, float(F(t[0]) + F(0.37) * F(j + 1)), float(F(t[1]) - F(0.61)), float(F(0.731) * F(j) - F(2.9))))
        entries.append((6, float(F(path[(f + 11) % 1000][0]) + F(0.125)), float(F(path[(f + 11) % 1000][1]) + F(0.875)), float(F(7.77))))   # the later wins
        things = [dict(t) for t in base]
        for m, x, y, a in entries:
            things[m].update(x=F(x), y=F(y), angle=F(a))
        view = {"x": r[0], "y": r[1], "angle": r[2], "cos": r[3], "sin": r[4], "cos_neg": r[5], "sin_neg": r[6], "floor_height": r[7]}
        want = nf.render_frame(np_map, things, sprites, np_wad, nm, W, H, view)
        fl = scene.build_lists_poses(W, H, dg.make_views(path[[f]])[0], entries)
        got = np.frombuffer(world["emul"].draw_lists(W, H, fl)[0], dtype=np.uint8).reshape(H, W, 3)
        bad = np.argwhere(np.any(got != want, axis=2))
        assert len(bad) == 0, f"frame {f}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]})"
        plain = np.frombuffer(world["emul"].draw_lists(W, H, scene.build_lists(W, H, dg.make_views(path[[f]])[0]))[0], dtype=np.uint8).reshape(H, W, 3)
        changed += not np.array_equal(got, plain)
    assert changed > 0


def test_sectors_at_equals_the_model(world):
    xs, ys = mp.lookup_points(world["wad"])
    assert len(xs) > 2000
    got = world["scene"].sectors_at(xs, ys)
    want = mp.model_sectors(world["wad"], xs, ys)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(xs)} points differ, first {np.argwhere(got != want)[0]}"
    assert (want >= 0).sum() > 1000 and len(set(want.tolist())) > 50


def test_sectors_at_on_the_partition_line_of_the_hand_world(dg):
    """mobj_pose_cases.line_points: where the side test is 0.0 and a fused one is not (sector 0 by the rule, 1 fused), and exact ties."""
    xs, ys, n = mp.line_points()
    scene = dg.Scene(mp.fc.wad_of("hand"), "e1m1")
    got = scene.sectors_at(xs, ys)
    assert np.array_equal(got, mp.line_sectors(xs, ys)), np.flatnonzero(got != mp.line_sectors(xs, ys))
    assert (got[:n] == 0).all()
    scene.close()


@pytest.fixture(scope="module")
def holes(dg, wad1993):
    wad = walk_cases.holes_wad(wad1993)
    return wad, dg.Scene(wad, "e1m1")


def test_sectors_at_on_a_map_with_holes(holes):
    wad, scene = holes
    xs, ys = mp.lookup_points(wad, seed=11)
    ring = walk_cases.far_ring(90)
    xs, ys = np.concatenate([xs, ring[:, 0]]), np.concatenate([ys, ring[:, 1]])
    got = scene.sectors_at(xs, ys)
    want = mp.model_sectors(wad, xs, ys)
    assert np.array_equal(got, want)
    assert (want < 0).sum() > 200 and (want >= 0).sum() > 1000


def test_an_object_moved_into_no_sector_is_not_drawn(dg, oracle, holes, path1993):
    """get_sector_from_vertex gives None for the object's new position: draw_map_objects skips it (map_objects.rs:100-104).  The oracle
    says so for the patched WAD, and no draw record carries the object's tag."""
    wad, scene = holes
    emul = emul_bind.EmulScene(wad)
    placed = scene.mobj_poses()
    path = path1993
    checked = 0
    for f in (100, 323, 640):
        view = dg.make_views(path[[f]])[0]
        fl0, own0 = scene.build_lists_owners(W, H, view)
        seen = sorted({int(t) & 0xFFFF for t in own0 if int(t) >> 16 == dg.DG_LABEL_MOBJ})
        if not seen:
            continue
        m = seen[0]
        # a whole-unit point near the camera that lies in no sector
        cand = [(int(path[(f + d) % 1000][0]) + ox, int(path[(f + d) % 1000][1]) + oy) for d in range(0, 60, 3) for ox in (0, 24, -24) for oy in (0, 24, -24)]
        sec = scene.sectors_at([c[0] for c in cand], [c[1] for c in cand])
        assert (sec < 0).any()
        x, y = cand[int(np.argmax(sec < 0))]
        entries = [(m, x, y, 90)]
        fl, own = scene.build_lists_poses(W, H, view, mp.entries_as_poses(entries), owners=True)
        assert m not in {int(t) & 0xFFFF for t in own if int(t) >> 16 == dg.DG_LABEL_MOBJ}
        got = emul.draw_lists(W, H, fl)[0]
        osc = oracle.Scene(mp.patch_things(wad, mp.resolved(entries)), "e1m1")
        assert got == osc.render(W, H, path[f])
        osc.close()
        assert placed["sector"][m] >= 0
        checked += 1
    assert checked >= 2


def test_argument_errors(dg, world):
    L, scene = dg.lib(), world["scene"]
    n = scene.mobj_count()
    view = dg.make_views(world["path"][[0]])[0]
    fl = dg.DgFrameLists()
    for bad in (n, n + 7, -1, 1 << 20):
        with pytest.raises(dg.DoomGpuError) as e:
            scene.build_lists_poses(W, H, view, [(0, 100.0, 100.0, 0.0), (bad, 100.0, 100.0, 0.0)])
        assert e.value.code == dg.DG_ERR_INVALID and "map object index out of range" in str(e.value)
    vp = dg.DgViewPoses(None, 3)
    assert L.dg_build_lists_poses(scene._h, W, H, ctypes.byref(view), ctypes.byref(vp), ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_poses(None, W, H, ctypes.byref(view), None, ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_poses(scene._h, W, H, None, None, ctypes.byref(fl), None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_poses(scene._h, W, H, ctypes.byref(view), None, None, None) == dg.DG_ERR_INVALID
    assert L.dg_build_lists_poses(scene._h, W, H, ctypes.byref(view), None, ctypes.byref(fl), None) == dg.DG_OK
    out = np.zeros(n + 1, dtype=dg.MOBJ_PLACED_DTYPE)
    for bad_n in (n - 1, n + 1, 0, -1):
        assert L.dg_scene_mobj_poses(scene._h, out.ctypes.data, bad_n) == dg.DG_ERR_INVALID
    assert L.dg_scene_mobj_poses(None, out.ctypes.data, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_mobj_poses(scene._h, None, n) == dg.DG_ERR_INVALID
    assert L.dg_scene_mobj_poses(scene._h, out.ctypes.data, n) == dg.DG_OK
    x = np.zeros(4, dtype=np.float32)
    s = np.zeros(4, dtype=np.int32)
    assert L.dg_scene_sectors_at(None, x.ctypes.data, x.ctypes.data, 4, s.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_scene_sectors_at(scene._h, None, x.ctypes.data, 4, s.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_scene_sectors_at(scene._h, x.ctypes.data, None, 4, s.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_scene_sectors_at(scene._h, x.ctypes.data, x.ctypes.data, 4, None) == dg.DG_ERR_INVALID
    assert L.dg_scene_sectors_at(scene._h, x.ctypes.data, x.ctypes.data, -1, s.ctypes.data) == dg.DG_ERR_INVALID
    assert L.dg_scene_sectors_at(scene._h, None, None, 0, None) == dg.DG_OK
    assert (dg.DG_ERR_STATE, ctypes.sizeof(dg.DgMobjPose), ctypes.sizeof(dg.DgMobjPlaced), dg.MOBJ_PLACED_DTYPE.itemsize) == (-7, 16, 16, 16)
    assert ctypes.sizeof(dg.DgViewPoses) == 16 and b"ABI 4" in L.dg_version()


def test_the_pose_bodies_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/mobj_pose/mobj_pose_host_main.cpp (its own main) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: view_rows_core.h's fill and scatter bodies for the pose kind lane after lane at the kernels' boundary
    counts against Scene::sector_from_vertex, then the host walker with poses.  It checks its own results; any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "mobj_pose_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "mobj_pose", "mobj_pose_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    for name, data in (("light.wad", wad1993), ("holes.wad", walk_cases.holes_wad(wad1993))):
        wad = tmp_path / name
        wad.write_bytes(data)
        r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                           capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
        assert r.returncode == 0 and "mobj_pose_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
