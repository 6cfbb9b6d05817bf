"""CPU tier of the bundle submission: dg_bundle_lists_host (the binner + csrc/plane_core.h on the CPU — the rule dg_bundle_tiles
evaluates, and what the GPU path is tested against in test_bundle_gpu.py) must equal dg_depth_lists_host and dg_label_lists_host, which
test_depth_host.py and test_labels_host.py hold against the numpy models, plane for plane and box for box; the three share their code, so
the hand-built lists are also held against the numpy models (np_depth, np_labels) directly; and dg_bundle_layout must be the layout
DESIGN.md §8i states.

  whole frames    dg_build_lists_owners output of the light map, the vanilla-shaped map and the hand-packed IWAD at 160x100, 131x67, 5x9
  hand-built      every case of tests/depth_cases.py with test_labels_host's hand-given owners: the 70-span column, 24 records per column,
                  the all-transparent masked column, x >= W, the 1-row skip
  outputs         each of the five outputs NULL in turn, and each alone
  layout          order, 256-byte alignment, total, absent parts, even offsets of the 16-bit planes where 3nWH is odd, the capacity rule
                  against a Python restatement
  errors          every error return of dg_bundle_lists_host and dg_bundle_layout
  stand-alone     tests/bundle/bundle_host_main.cpp: the host entries on a frame built by hand under AddressSanitizer + UBSan, as a program
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import depth_cases
from test_depth_host import SIZES, _map_views
from test_edge_kats import to_dg_lists, view_dict
from test_labels_host import hand_owners

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NAMES = ("distance", "kind", "id", "cls", "boxes")
HAND_SIZES = ((64, 40), (131, 67), (5, 9))


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {len(bad)} {name} entries differ, first at {bad[0].tolist()}: bundle {g[tuple(bad[0])]} separate {w[tuple(bad[0])]}"


def _separate(dg, scene, W, H, frames, owners):
    return tuple(dg.depth_lists_host(scene, W, H, frames)) + tuple(dg.label_lists_host(scene, W, H, frames, owners))


@pytest.mark.parametrize("which", ["light", "vanilla", "hand"])
def test_whole_frames_equal_the_two_host_functions(dg, campath_mod, wad1993, wad1995, path1993, path1995, which):
    wad, views = _map_views(dg, campath_mod, which, wad1993, wad1995, path1993, path1995)
    scene = dg.Scene(wad, "e1m1")
    seen_cls, seen_kind, mobj_pixels, n = set(), set(), 0, 0
    for (W, H, k) in SIZES:
        for v in views[:k]:
            fl, owners = scene.build_lists_owners(W, H, v)
            frames = (dg.DgFrameLists * 1)(fl)
            want = _separate(dg, scene, W, H, frames, [owners])
            _same(dg.bundle_lists_host(scene, W, H, frames, [owners]), want, f"{which} {W}x{H}")
            seen_cls |= set(np.unique(want[3]).tolist())
            seen_kind |= set(np.unique(want[1]).tolist())
            mobj_pixels += int(want[4]["pixels"].sum())
            n += 1
    assert n == 7 and {1, 2, 3, 4} <= seen_cls and {1, 2, 3} <= seen_kind and mobj_pixels > 0       # none of it passes vacuously
    scene.close()


@pytest.fixture(scope="module")
def hand_built(dg, campath_mod, wad1993):
    """{(W, H): (frames, owners, the separate host functions' outputs)} of every depth_cases case at the size, and the scene."""
    import np_front_end as nf
    scene = dg.Scene(wad1993, "e1m1")
    n_segs, n_mobjs = len(nf.Map(wad1993, "e1m1").segs), scene.mobj_count()
    out, keep = {}, []
    for (W, H) in HAND_SIZES:
        cs = depth_cases.cases(W, H)
        frames, owners = (dg.DgFrameLists * len(cs))(), []
        for i, (name, v, lists) in enumerate(cs):
            rec, _vd = view_dict(campath_mod, *v)
            frames[i], k = to_dg_lists(dg, scene, rec, lists)
            keep.append(k)
            owners.append(hand_owners(dg, lists, n_segs, n_mobjs))
        out[(W, H)] = (frames, owners, _separate(dg, scene, W, H, frames, owners), [c[0] for c in cs])
    yield out, scene
    scene.close()
    del keep


def test_hand_built_lists_equal_the_two_host_functions(dg, hand_built):
    cases, scene = hand_built
    assert cases[(64, 40)][3] == ["horizon", "wall_corners", "masked_over_floor", "dense_strip", "seventy"] and "seventy" not in cases[(5, 9)][3]
    for (W, H), (frames, owners, want, names) in cases.items():
        _same(dg.bundle_lists_host(scene, W, H, frames, owners), want, f"hand-built {W}x{H}")
        for i, name in enumerate(names):
            assert (want[3][i] != 0).any() and (want[1][i] != 0).any(), f"{name} {W}x{H} draws nothing"
        assert (want[3] == 2).any() and (want[4]["pixels"] > 0).any()
    # what the cases are there for, on the expected data: a column with more spans than the kernels stage, the vy == 0 row's three values
    frames, owners, want, names = cases[(64, 40)]
    hz = want[0][names.index("horizon")][20]
    assert {-32768, 32767, 0} <= set(hz.tolist())


def test_hand_built_lists_equal_the_numpy_models(dg, hand_built, wad1993):
    """All five outputs of one dg_bundle_lists_host call against np_depth / np_labels, which share nothing with the library."""
    import np_depth
    import np_front_end as nf
    import np_labels as nl
    cases, scene = hand_built
    names, n_mobjs = np_depth.SceneNames(dg, scene, wad1993, nf), scene.mobj_count()
    for (W, H), (frames, owners, _want, case_names) in cases.items():
        got = dg.bundle_lists_host(scene, W, H, frames, owners)
        for i, name in enumerate(case_names):
            dist, kind, _tr = np_depth.depth_of_frame_lists(names, "SKY1", W, H, frames[i])
            ids, cls, boxes, _tr, kind2 = nl.labels_of_frame_lists(names, "SKY1", W, H, frames[i], owners[i], n_mobjs)
            assert np.array_equal(kind, kind2)
            for plane, g, w in zip(NAMES, got, (dist, kind, ids, cls, boxes)):
                bad = np.argwhere(g[i] != w)
                assert g[i].shape == w.shape and len(bad) == 0, f"{name} {W}x{H} {plane}: {len(bad)} differ from the numpy model, first at {bad[:1].tolist()}"


def test_each_output_may_be_left_out_and_each_may_stand_alone(dg, hand_built):
    cases, scene = hand_built
    W, H = 64, 40
    frames, owners, want, _n = cases[(W, H)]
    for k in range(5):
        for alone in (False, True):
            flags = [(i == k) == alone for i in range(5)]
            got = dg.bundle_lists_host(scene, W, H, frames, owners, *flags)
            assert [g is not None for g in got] == flags
            for i in range(5):
                if flags[i]:
                    assert np.array_equal(got[i], want[i]), (NAMES[k], alone, NAMES[i])
    # the depth planes need no owner tags
    got = dg.bundle_lists_host(scene, W, H, frames, None, True, True, False, False, False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- layout -------------------------------------------------------------------------------------------------------------------------------

def _layout(W, H, n, what):
    """DESIGN.md §8i restated: colour 3nWH | distance 2nWH | kind nWH | id 2nWH | cls nWH, the requested parts only, each on a 256-byte
    boundary; total = the end of the last part; a part that is not there sits at total."""
    px, at, end, off = n * W * H, 0, 0, {}
    for bit, parts in ((1, (("colour", 3),)), (2, (("distance", 2), ("kind", 1))), (4, (("id", 2), ("cls", 1)))):
        for name, b in parts:
            if what & bit:
                off[name] = at
                end = at + b * px
                at = (end + 255) // 256 * 256
            else:
                off[name] = None
    return {k: (end if v is None else v) for k, v in off.items()} | {"total": end}


@pytest.mark.parametrize("what", range(1, 8))
def test_the_layout_of_every_what(dg, what):
    for (W, H, n) in ((5, 9, 3), (131, 67, 7), (1280, 800, 333), (64, 40, 1), (1, 1, 1)):
        L = dg.bundle_layout(W, H, n, what)
        assert L == _layout(W, H, n, what), (W, H, n)
        px = n * W * H
        present = [(k, b) for k, b, bit in (("colour", 3, 1), ("distance", 2, 2), ("kind", 1, 2), ("id", 2, 4), ("cls", 1, 4)) if what & bit]
        absent = [k for k, bit in (("colour", 1), ("distance", 2), ("kind", 2), ("id", 4), ("cls", 4)) if not what & bit]
        assert all(L[k] == L["total"] for k in absent)
        assert all(L[k] % 256 == 0 for k, _b in present) and L[present[0][0]] == 0
        for (a, ab), (b, _bb) in zip(present, present[1:]):              # in order, not overlapping, no more than the alignment apart
            assert L[a] + ab * px <= L[b] < L[a] + ab * px + 256
        assert L["total"] == L[present[-1][0]] + present[-1][1] * px
    L = dg.bundle_layout(5, 9, 3, what)                                  # 3nWH = 405 is odd: the 16-bit planes still sit on even offsets
    assert (not what & 2 or L["distance"] % 2 == 0) and (not what & 4 or L["id"] % 2 == 0)
    if what & 1 and what != 1:
        assert min(L[k] for k in ("distance", "id")) == 512              # (405 rounded up, not 405)
    if what == 7:
        assert L == {"colour": 0, "distance": 512, "kind": 1024, "id": 1280, "cls": 1792, "total": 1792 + 135}


@pytest.mark.parametrize("what", range(1, 8))
def test_the_capacity_rule_against_the_restated_layout(dg, what):
    """dg_bundle_capacity needs a ctx; its rule — the largest n <= max_batch whose total fits max_batch * 3WH — is checked here on
    dg_bundle_layout itself (test_bundle_gpu.py holds the ctx's answer against the same search)."""
    for (W, H, max_batch) in ((5, 9, 3), (5, 9, 11), (131, 67, 16), (1280, 800, 1000), (320, 200, 1)):
        slab = max_batch * 3 * W * H
        fits = [n for n in range(1, max_batch + 1) if dg.bundle_layout(W, H, n, what)["total"] <= slab]
        cap = max(fits, default=0)
        assert fits == list(range(1, cap + 1))                            # total grows with n: what fits is a prefix
        assert cap == max([n for n in range(1, max_batch + 1) if _layout(W, H, n, what)["total"] <= slab], default=0)
        if cap < max_batch:
            assert dg.bundle_layout(W, H, cap + 1, what)["total"] > slab
        if what == 1:
            assert cap == max_batch                                       # colour alone is a colour submission's slab
        if what == 7 and max_batch == 1000:
            assert cap == 333                                             # about max_batch / 3 for all three parts
    assert max([n for n in range(1, 4) if dg.bundle_layout(5, 9, n, 7)["total"] <= 3 * 135], default=0) == 0     # a ctx too small for even one frame


# ---- errors -------------------------------------------------------------------------------------------------------------------------------

def test_every_error_return_of_the_host_only_calls(dg, hand_built):
    L = dg.lib()
    cases, scene = hand_built
    W, H = 64, 40
    frames4, owners4, want, _n = cases[(W, H)]
    frames = (dg.DgFrameLists * 1)(frames4[0])
    owners = owners4[0]
    op, keep = dg.owner_pointers([owners])
    dist, kind = np.full((1, H, W), 77, dtype=np.int16), np.full((1, H, W), 77, dtype=np.uint8)
    ids, cls = np.full((1, H, W), 77, dtype=np.uint16), np.full((1, H, W), 77, dtype=np.uint8)
    boxes = np.zeros((1, scene.mobj_count()), dtype=dg.LABEL_BOX_DTYPE)
    boxes["pixels"] = 77
    outs = [a.ctypes.data_as(P) for a in (dist, kind, ids, cls, boxes)]

    def untouched():
        return all((a == 77).all() for a in (dist, kind, ids, cls)) and (boxes["pixels"] == 77).all()

    call = L.dg_bundle_lists_host
    assert call(None, W, H, frames, op, 1, *outs) == dg.DG_ERR_INVALID
    assert call(scene._h, W, H, None, op, 1, *outs) == dg.DG_ERR_INVALID
    for (w, h) in ((0, 40), (64, 0), (-1, 40), (64, -3), (16385, 40), (64, 16385)):
        assert call(scene._h, w, h, frames, op, 1, *outs) == dg.DG_ERR_INVALID, (w, h)
    assert call(scene._h, W, H, frames, op, -1, *outs) == dg.DG_ERR_INVALID
    # labels without owners: any one label output is enough to need them; the depth outputs alone are not
    for k in (2, 3, 4):
        only = [o if i == k else None for i, o in enumerate(outs)]
        assert call(scene._h, W, H, frames, None, 1, *only) == dg.DG_ERR_INVALID, NAMES[k]
        assert b"owners" in L.dg_last_error()
    null_op, _k = dg.owner_pointers([None])
    assert call(scene._h, W, H, frames, null_op, 1, *outs) == dg.DG_ERR_INVALID
    # a bad tag names its frame
    for tag in (dg.owner_tag(0, 0), dg.owner_tag(3, 0), dg.owner_tag(2, scene.mobj_count()), dg.owner_tag(1, 0xFFFF), 0xFFFFFFFF):
        bad = owners.copy()
        bad[-1] = tag
        bad_op, _k = dg.owner_pointers([bad])
        assert call(scene._h, W, H, frames, bad_op, 1, *outs) == dg.DG_ERR_INVALID, hex(tag)
        assert b"frame 0" in L.dg_last_error()
        two_op, _k = dg.owner_pointers([owners, bad])
        cls2 = np.full((2, H, W), 77, dtype=np.uint8)
        assert call(scene._h, W, H, (dg.DgFrameLists * 2)(frames[0], frames[0]), two_op, 2, None, None, None, cls2.ctypes.data_as(P), None) == dg.DG_ERR_INVALID
        assert (cls2 == 77).all()
        assert b"frame 1" in L.dg_last_error()
    # malformed lists are the binner's errors
    broken = (dg.DgFrameLists * 1)(frames[0])
    broken[0].n_renders = 0
    assert call(scene._h, W, H, broken, op, 1, *outs) == dg.DG_ERR_INVALID
    assert untouched()                                                    # nothing was written by a refused call
    assert call(scene._h, W, H, frames, op, 0, *outs) == dg.DG_OK and untouched()
    assert call(scene._h, W, H, frames, op, 1, None, None, None, None, None) == dg.DG_OK
    assert call(scene._h, W, H, frames, op, 1, *outs) == dg.DG_OK
    assert all(np.array_equal(a[0], w[0]) for a, w in zip((dist, kind, ids, cls, boxes), want))
    # dg_bundle_layout
    o = dg.DgBundleOffsets()
    o.total = 77
    lay = L.dg_bundle_layout
    assert lay(W, H, 1, 7, None) == dg.DG_ERR_INVALID
    for what in (0, 8, 15, 0x80000001, 0xFFFFFFFF):
        assert lay(W, H, 1, what, ctypes.byref(o)) == dg.DG_ERR_INVALID, what
    for (w, h, n) in ((0, 40, 1), (64, 0, 1), (-1, 40, 1), (64, -3, 1), (16385, 40, 1), (64, 16385, 1), (64, 40, 0), (64, 40, -2)):
        assert lay(w, h, n, 7, ctypes.byref(o)) == dg.DG_ERR_INVALID, (w, h, n)
    assert o.total == 77
    assert lay(W, H, 1, 7, ctypes.byref(o)) == dg.DG_OK and o.total == 9 * 2560                     # 7680 | 5120 | 2560 | 5120 | 2560, all multiples of 256
    del keep


def test_the_binding_and_the_header_carry_the_bundle_entry_points(dg):
    declared = dg.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", dg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in ("dg_bundle_layout", "dg_bundle_capacity", "dg_submit_bundle_views", "dg_bundle_lists", "dg_bundle_lists_host", "dg_slot_bundle_timing"):
        assert n in declared and n in exported and n in dg._SIGNATURES and hasattr(dg.lib(), n), n
    assert (dg.DG_FE_BUNDLE, dg.DG_BUNDLE_COLOUR, dg.DG_BUNDLE_DEPTH, dg.DG_BUNDLE_LABELS) == (7, 1, 2, 4)
    hdr = open(dg.INCLUDE).read()
    for line in ("#define DG_FE_BUNDLE 7", "#define DG_BUNDLE_COLOUR 1u", "#define DG_BUNDLE_DEPTH  2u", "#define DG_BUNDLE_LABELS 4u"):
        assert line in hdr, line
    assert ctypes.sizeof(dg.DgBundleOffsets) == 48
    for n in ("submit_bundle", "bundle_lists", "bundle_capacity", "bundle_timing"):
        assert callable(getattr(dg.Context, n)), n
    assert callable(dg.bundle_layout) and callable(dg.bundle_lists_host)
    assert b"ABI 4" in dg.lib().dg_version()


def test_the_host_entries_as_a_stand_alone_program_under_sanitizers(tmp_path, wad1993):
    """tests/bundle/bundle_host_main.cpp (its own main, the C-ABI alone) with the host sources of the library, built with
    -fsanitize=address,undefined and run as a program: it checks its own results, and any sanitizer report fails it."""
    csrc = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
    exe = tmp_path / "bundle_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "bundle", "bundle_host_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("api_scene.cpp", "scene.cpp", "frontend.cpp", "binner.cpp", "walk.cpp")])
    wad = tmp_path / "light.wad"
    wad.write_bytes(wad1993)
    r = subprocess.run([str(exe), str(wad), os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), "e1m1"],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "bundle_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
