"""CPU tier of the line-of-sight queries: dg_sight_host and dg_sight_mobjs_host against np_sight's two
restatements of the rule, the doors, the errors, the exports, and tests/sight/sight_host_main.cpp — sight_core.h's traversal in the
device's form — as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import np_sight as ns
import sight_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EYE = 41.0
NEW_SYMBOLS = ("dg_sight_host", "dg_sight_device", "dg_sight_words", "dg_sight_mobjs_host", "dg_sight_mobjs_device", "dg_ctx_sight_kernel_ms", "dg_scene_bsp_depth")


@pytest.fixture(scope="module")
def scenes(dg):
    made = {}

    def get(world):
        if world not in made:
            made[world] = dg.Scene(sc.wad_of(world), "e1m1")
        return made[world]
    yield get
    for s in made.values():
        s.close()


# ---- 1. the host twin against model (a) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", sc.WORLDS)
def test_host_twin_equals_the_rule_on_every_family(dg, scenes, world):
    m = sc.model_of(world)
    heights = m.height_rows(1)
    for name, q in sc.families(world).items():
        want = m.visible(q, heights)
        got = dg.sight_host(scenes(world), q)
        assert np.array_equal(got, want), (world, name, np.flatnonzero(got != want)[:8].tolist())
        print(f"{world:6s} {name:13s} {len(q):4d} queries, {int(want.sum()):4d} visible")
        # what a family can show, it shows: both answers, or the one answer it is about
        if name in ("random", "near", "partition", "vertex", "slit") or (name == "on_two_sided" and world != "hand"):     # (the hand world has one two-sided line)
            assert 0 < want.sum() < len(q), (world, name, int(want.sum()))
        if name == "empty_range":
            assert not want[0::3].any() and not want[1::3].any() and want[2::3].any(), (world, name)
        if name == "contract":
            bad = ~m.in_contract(q)
            # in contract and visible: the base hop, and the two that only widen its target range (z1_lo = -65536, z1_hi = 65536)
            assert bad.sum() == 7 * 6 and not want[bad].any() and want[0] == 1 and want[~bad].sum() >= 3, (world, name)
    assert scenes(world).bsp_depth() == m.depth()


def test_the_slit_family_has_both_answers_on_each_side_of_an_edge():
    """Per stepped line the slit family holds, for each edge, five target ranges from one unit outside to one unit inside what the slit
    lets through: the model says "not visible" for some and "visible" for others of the same line."""
    m = sc.model_of("hand")
    q = sc.families("hand")["slit"]
    v = m.visible(q, m.height_rows(1)).reshape(-1, 5, 3)
    assert (v.any(axis=1) & ~v.all(axis=1)).any(), v.tolist()


# ---- 2. model (a) against model (b) ------------------------------------------------------------------------------------------------------

def exact_outcomes(world, seed):
    m = sc.model_of(world)
    q = sc.exact_queries(world, 1500, seed)
    heights = m.height_rows(1)
    a, zero_a = m.model_a(q, heights, details=True)
    b, zero_b = m.model_b(q, heights, details=True)
    return q, a, b, ~(zero_a | zero_b)


def test_on_the_holes_world_the_rule_sees_what_brute_force_sees_and_more():
    """The holes world's emptied subsectors leave linedef stretches without a seg: a sight line crosses them unhindered by the rule and
    is stopped by the brute-force model, which knows every linedef.  So this world is left out of the comparison below (DESIGN.md
    section 8v records it); what still holds is the one direction — the rule looks at a subset of the linedefs and every step only
    closes a query further, so whatever brute force calls visible the rule calls visible — and every disagreement is a line that passes
    through an emptied leaf."""
    m = sc.model_of("holes")
    q, a, b, keep = exact_outcomes("holes", 6)
    differ = keep & ((a == ns.VISIBLE) != (b == ns.VISIBLE))
    print("holes: kept", int(keep.sum()), "disagree", int(differ.sum()))
    assert differ.any() and ((a == ns.VISIBLE) | (b != ns.VISIBLE))[keep].all()
    at_leaf, _ = m.visited_leaves(q)
    emptied = m.leaf_count == 0
    assert at_leaf[emptied][:, differ].any(axis=0).all()


@pytest.mark.parametrize("world,seed", [("e1m1", 5), ("hand", 7)])
def test_rule_equals_brute_force_where_every_cross_product_is_exact(world, seed):
    """Endpoints k + 0.5 inside the map's box, E at most EXACT_SPAN from S per axis.  The bound: map vertices and partition vectors are
    whole numbers, so every factor of a cross product is a multiple of 1/2 and every product a multiple of 1/2 (a half-integer times a
    whole number: d, l and b are differences of like numbers); the factors are bounded by the box (below 4161 per axis on every world)
    times the longest of EXACT_SPAN, a linedef's extent and a partition vector's extent, asserted below to keep every product under
    2^22 — then both products and their difference are multiples of 1/2 below 2^23: exact in f32."""
    m = sc.model_of(world)
    box = max(float(m.vx.max() - m.vx.min()), float(m.vy.max() - m.vy.min())) + 1.0
    longest = max(float(sc.EXACT_SPAN[world]), float(np.abs(m.vx[m.line_v2] - m.vx[m.line_v1]).max()), float(np.abs(m.vy[m.line_v2] - m.vy[m.line_v1]).max()),
                  float(np.abs(m.node[:, 2:]).max()))
    far = max(box, float(np.abs(m.node[:, :2]).max()) + box)                     # |S - A|, |S - n|: inside the box, or from a partition's origin
    assert far * longest < 2.0 ** 22, (world, far, longest)
    q, a, b, keep = exact_outcomes(world, seed)
    shares = {k: float((b[keep] == v).mean()) for k, v in (("visible", ns.VISIBLE), ("one_sided", ns.ONE_SIDED), ("closed", ns.CLOSED))}
    print(world, "kept", int(keep.sum()), "of", len(q), shares)
    assert keep.mean() >= 0.9, (world, float(keep.mean()))
    assert min(shares.values()) >= 0.05, (world, shares)
    assert np.array_equal(a[keep] == ns.VISIBLE, b[keep] == ns.VISIBLE), (world, np.flatnonzero(keep & ((a == ns.VISIBLE) != (b == ns.VISIBLE)))[:8].tolist())


# ---- 3. doors ------------------------------------------------------------------------------------------------------------------------------

def test_a_door_shut_in_one_frame_blocks_there_alone(dg, scenes):
    pair, sector, shut = sc.hand_door()
    m = sc.model_of("hand")
    opened = (sector, int(m.heights[sector, 0]), int(m.heights[sector, 1]))
    q = np.repeat(pair, 3)
    q["frame"] = [0, 1, 2]
    entries = [[], [opened, shut], [shut, opened]]                             # of two entries for one sector the later wins
    sectors, keep = dg.make_view_sectors(entries)
    got = dg.sight_host(scenes("hand"), q, sectors, 3)
    assert got.tolist() == [1, 0, 1]
    assert np.array_equal(got, m.visible(q, m.height_rows(3, entries)))
    assert dg.sight_host(scenes("hand"), q, None, 3).tolist() == [1, 1, 1]
    # the other order of the frames' queries, and the door shut everywhere
    assert dg.sight_host(scenes("hand"), q[::-1].copy(), sectors, 3).tolist() == [1, 0, 1]
    all_shut, keep2 = dg.make_view_sectors([[shut]] * 3)
    assert dg.sight_host(scenes("hand"), q, all_shut, 3).tolist() == [0, 0, 0]
    del keep, keep2


# ---- 4. the mobjs form -----------------------------------------------------------------------------------------------------------------------

def mobj_queries(dg, scene, m, views, heights_f32, poses, entries):
    """The queries dg_sight_mobjs stands for, assembled in numpy: (queries, (frame, mobj) of each)."""
    placed = scene.mobj_poses()
    n_frames = len(views)
    assert np.array_equal(scene.sector_heights().astype(np.int64), m.heights)
    rows = m.height_rows(n_frames, entries)
    out, who = [], []
    for f in range(n_frames):
        x, y, sector = placed["x"].copy(), placed["y"].copy(), placed["sector"].copy()
        for (mo, px, py, _) in (poses[f] if poses else []):
            x[mo], y[mo] = F(px), F(py)
            sector[mo] = scene.sectors_at([x[mo]], [y[mo]])[0]
        z0 = F(F(views[f].floor_height) + F(EYE))
        for mo in range(len(placed)):
            if sector[mo] < 0 or not heights_f32[mo] > 0:
                continue
            lo = F(rows[f, sector[mo], 0])
            out.append((f, F(views[f].x), F(views[f].y), z0, x[mo], y[mo], lo, F(lo + heights_f32[mo])))
            who.append((f, mo))
    return ns.queries(out), who


def bits_of(words, n_frames, results, who):
    rows = np.zeros((n_frames, words), dtype=np.uint32)
    for r, (f, mo) in zip(results, who):
        if r:
            rows[f, mo >> 5] |= np.uint32(1 << (mo & 31))
    return rows


def mobj_case(dg, world):
    """(views, poses, entries) of a world: viewers inside the map; in the frames with poses an object moved into another sector, one to a
    point in no sector (the holes world has such points) and one behind the door the frame's sector entry shuts."""
    m = sc.model_of(world)
    if world == "hand":
        spots = [(96.0, 180.0, 0.0), (250.0, 300.0, 0.0), (600.0, 250.0, 24.0), (96.0, 180.0, 0.0)]
        poses = [[], [(1, 600.0, 200.0, 0.5), (2, 100.0, 100.0, 0.0), (1, 500.0, 300.0, 1.0)], [(0, 300.0, 200.0, 0.0)], [(2, 700.0, 300.0, 0.0)]]
        entries = [[], [], [(1, 24, 24)], [(1, 104, 104), (0, 0, 100)]]                        # frame 3: object 2 moved behind the shut door
    else:
        path = np.fromfile(os.path.join(ROOT, "tests", "golden", "campath_seed1993.f32"), dtype="<f4").reshape(1000, 8)
        spots = [(float(r[0]), float(r[1]), float(r[7])) for r in path[[0, 297, 623, 728, 900]]]
        far = (2048.0 + 30000.0, 1536.0, 0.0)
        poses = [[], [(3, spots[2][0], spots[2][1], 0.0), (5, *far), (3, spots[3][0] + 8.0, spots[3][1], 0.0)], [], [(0, spots[0][0] + 32.0, spots[0][1] + 16.0, 0.0)], [(9, *far)]]
        two = [int(l) for l in range(len(m.line_v1)) if m.line_flags[l] & 4 and m.line_front[l] >= 0 and m.line_back[l] >= 0]
        doors = sorted({int(m.line_back[l]) for l in two[:40]})[:6]
        entries = [[], [(s, int(m.heights[s, 1]), int(m.heights[s, 1])) for s in doors], [(doors[0], 0, 0), (doors[0], 8, 120)], [], []]
    views = (dg.DgView * len(spots))(*[dg.DgView(x, y, 0.0, fl, 0, 0, 0, 0, 0.0, 0) for x, y, fl in spots])
    return views, poses, entries


@pytest.mark.parametrize("world", ["holes", "hand"])
@pytest.mark.parametrize("with_poses,with_entries", [(False, False), (True, False), (False, True), (True, True)])
def test_mobjs_form_equals_the_queries_it_stands_for(dg, scenes, world, with_poses, with_entries):
    scene, m = scenes(world), sc.model_of(world)
    views, poses, entries = mobj_case(dg, world)
    n, n_mobjs = len(views), scene.mobj_count()
    heights = sc.mobj_heights(n_mobjs)
    pa, keep_p = dg.make_view_poses(poses) if with_poses else (None, None)
    sa, keep_s = dg.make_view_sectors(entries) if with_entries else (None, None)
    got = dg.sight_mobjs_host(scene, views, EYE, heights, pa, sa)
    q, who = mobj_queries(dg, scene, m, views, heights, poses if with_poses else None, entries if with_entries else None)
    results = dg.sight_host(scene, q, sa, n)
    want = bits_of(got.shape[1], n, results, who)
    assert got.shape == (n, (n_mobjs + 31) // 32) and np.array_equal(got, want), (world, with_poses, with_entries)
    assert results.any(), world
    if world == "holes" or with_entries:                       # (the hand world's two rooms are open to each other until a door shuts)
        assert not results.all(), world
    tail = n_mobjs % 32
    if tail:
        assert not (got[:, -1] >> np.uint32(tail)).any()
    left_out = np.flatnonzero(~(heights > 0))
    assert len(left_out) and not any((got[:, mo >> 5] >> np.uint32(mo & 31) & 1).any() for mo in left_out)
    if with_poses and world == "holes":                        # the objects moved to a point in no sector are not seen
        assert scene.sectors_at([32048.0], [1536.0])[0] == -1
        assert not (got[1, 5 >> 5] >> np.uint32(5) & 1) and not (got[4, 9 >> 5] >> np.uint32(9) & 1)
    if with_poses and world == "hand":                         # object 2 in room B: seen through the portal, and not once the door is shut
        assert (got[3, 0] >> np.uint32(2) & 1) == (0 if with_entries else 1)
    del keep_p, keep_s


def test_mobjs_form_reads_moved_sectors_and_later_entries(dg, scenes):
    """An object moved into another sector stands on that sector's floor: with a tall step between the rooms the result changes with
    the sector, and of two poses of one object the later counts."""
    scene = scenes("hand")
    views = (dg.DgView * 1)(dg.DgView(96.0, 180.0, 0.0, 0.0, 0, 0, 0, 0, 0.0, 0))
    heights = np.full(scene.mobj_count(), 8.0, dtype=np.float32)
    pa, keep = dg.make_view_poses([[(2, 120.0, 200.0, 0.0), (2, 600.0, 250.0, 0.0)]])
    sa, keep2 = dg.make_view_sectors([[(1, 100, 128)]])                      # room B's floor far above the eye: an 8-unit object on it is hidden by the step
    assert dg.sight_mobjs_host(scene, views, EYE, heights, pa, None)[0, 0] >> np.uint32(2) & 1 == 1
    assert dg.sight_mobjs_host(scene, views, EYE, heights, pa, sa)[0, 0] >> np.uint32(2) & 1 == 0
    assert dg.sight_mobjs_host(scene, views, EYE, heights, None, sa)[0, 0] >> np.uint32(2) & 1 == 1       # as loaded it stands in room A
    del keep, keep2


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_are_refused(dg, scenes):
    L, scene = dg.lib(), scenes("hand")
    P = ctypes.c_void_p
    q = ns.queries([(0, 96.0, 180.0, 41.0, 100.0, 180.0, 0.0, 56.0)])
    out = np.zeros(4, dtype=np.uint8)
    qp, op = q.ctypes.data_as(P), out.ctypes.data_as(P)
    INVALID = dg.DG_ERR_INVALID
    assert L.dg_sight_host(None, None, 1, qp, 1, op) == INVALID
    assert L.dg_sight_host(scene._h, None, 1, None, 1, op) == INVALID
    assert L.dg_sight_host(scene._h, None, 1, qp, 1, None) == INVALID
    assert L.dg_sight_host(scene._h, None, 1, qp, -1, op) == INVALID
    assert L.dg_sight_host(scene._h, None, 1, None, 0, None) == dg.DG_OK                 # n == 0 does nothing
    for frame, n_frames in ((1, 1), (-1, 1), (0, 0), (3, 3)):
        bad = q.copy()
        bad["frame"] = frame
        assert L.dg_sight_host(scene._h, None, n_frames, bad.ctypes.data_as(P), 1, op) == INVALID, (frame, n_frames)
    for entry in ((2, 0, 10), (-1, 0, 10), (0, 40000, 10), (0, 0, -40000)):
        sa, keep = dg.make_view_sectors([[entry]])
        assert L.dg_sight_host(scene._h, sa, 1, qp, 1, op) == INVALID, entry
    null_entries = (dg.DgViewSectors * 1)(dg.DgViewSectors(None, 2))
    assert L.dg_sight_host(scene._h, null_entries, 1, qp, 1, op) == INVALID
    assert L.dg_sight_words(None) == INVALID and L.dg_scene_bsp_depth(None) == INVALID
    # the mobjs form
    views = (dg.DgView * 1)(dg.DgView(96.0, 180.0, 0.0, 0.0, 0, 0, 0, 0, 0.0, 0))
    h = np.full(scene.mobj_count(), 56.0, dtype=np.float32)
    rows = np.zeros((1, dg.lib().dg_sight_words(scene._h)), dtype=np.uint32)
    hp, rp = h.ctypes.data_as(P), rows.ctypes.data_as(P)
    assert L.dg_sight_mobjs_host(scene._h, views, None, None, 1, EYE, hp, rp) == dg.DG_OK
    assert L.dg_sight_mobjs_host(None, views, None, None, 1, EYE, hp, rp) == INVALID
    assert L.dg_sight_mobjs_host(scene._h, None, None, None, 1, EYE, hp, rp) == INVALID
    assert L.dg_sight_mobjs_host(scene._h, views, None, None, 1, EYE, None, rp) == INVALID
    assert L.dg_sight_mobjs_host(scene._h, views, None, None, 1, EYE, hp, None) == INVALID
    assert L.dg_sight_mobjs_host(scene._h, views, None, None, -1, EYE, hp, rp) == INVALID
    assert L.dg_sight_mobjs_host(scene._h, None, None, None, 0, EYE, None, None) == dg.DG_OK
    sa, keep = dg.make_view_sectors([[(7, 0, 10)]])
    assert L.dg_sight_mobjs_host(scene._h, views, None, sa, 1, EYE, hp, rp) == INVALID
    pa, keep2 = dg.make_view_poses([[(scene.mobj_count(), 0.0, 0.0, 0.0)]])
    assert L.dg_sight_mobjs_host(scene._h, views, pa, None, 1, EYE, hp, rp) == INVALID
    null_poses = (dg.DgViewPoses * 1)(dg.DgViewPoses(None, 1))
    assert L.dg_sight_mobjs_host(scene._h, views, null_poses, None, 1, EYE, hp, rp) == INVALID
    # the device calls and the timing getter without a ctx
    assert L.dg_sight_device(None, None, 1, qp, 1, op) == INVALID
    assert L.dg_sight_mobjs_device(None, views, None, None, 1, EYE, hp, rp) == INVALID
    a, b = ctypes.c_float(), ctypes.c_float()
    assert L.dg_ctx_sight_kernel_ms(None, ctypes.byref(a), ctypes.byref(b)) == INVALID
    assert b"ctx" in L.dg_last_error()


# ---- 6. exports ------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_exported_and_bound(dg):
    declared = dg.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", dg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in dg._SIGNATURES, name
    assert dg.SIGHT_QUERY_DTYPE == ns.QUERY_DTYPE and dg.SIGHT_QUERY_DTYPE.itemsize == 32
    header = open(os.path.join(ROOT, "include", "doomgpu.h")).read()
    assert "typedef struct dg_sight_query { int32_t frame; float x0, y0, z0, x1, y1, z1_lo, z1_hi; } dg_sight_query;" in header
    core = open(os.path.join(ROOT, "doom-rust-renderer_amd", "csrc", "sight_core.h")).read()
    assert f"constexpr uint32_t SIGHT_MAX_DEPTH = {sc.SIGHT_MAX_DEPTH};" in core


# ---- 7. the traversal in the device's form, as a stand-alone program under sanitizers --------------------------------------------------------

def tables_file(path, m, heights, q, expected):
    """The tables of tests/sight/sight_host_main.cpp's file format, from the model's lumps."""
    n_leaves, n_lines, n_sectors = len(m.leaf_count), len(m.line_v1), len(m.heights)
    child = np.where(m.child & 0x8000, ~(m.child & 0x7FFF), m.child).astype("<i4")
    nodes = b"".join(struct.pack("<ffffii", *[float(v) for v in m.node[i]], int(child[i, 0]), int(child[i, 1])) for i in range(m.n_nodes))
    leaves = b"".join(struct.pack("<IIi", int(m.leaf_first[l]), int(m.leaf_count[l]), -1) for l in range(n_leaves))
    lines = b"".join(struct.pack("<ffffiiII", float(m.vx[m.line_v1[l]]), float(m.vy[m.line_v1[l]]), float(m.vx[m.line_v2[l]]), float(m.vy[m.line_v2[l]]),
                                 int(m.line_front[l]), int(m.line_back[l]), int(m.line_flags[l]), 0) for l in range(n_lines))
    head = struct.pack("<9I", 0x31544753, m.n_nodes, n_leaves, len(m.seg_line), n_lines, n_sectors, heights.shape[0], len(q), m.depth())
    with open(path, "wb") as f:
        f.write(head + nodes + leaves + m.seg_line.astype("<u4").tobytes() + lines + heights.astype("<i2").tobytes() + q.tobytes() + expected.astype(np.uint8).tobytes())


def test_the_device_form_of_the_traversal_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/sight/sight_host_main.cpp (its own main, sight_core.h alone) built with -fsanitize=address,undefined and run as a program:
    dg_sight_queries as a host loop over lanes with SightLaneStack columns in a block of the kernel's LDS size, on tables, queries and
    expected results written here from the lumps and the model — the three worlds' families, the doors' three frames, and the chain
    BSPs at the capacity and one under it.  It checks its own results; any sanitizer report fails it."""
    exe = tmp_path / "sight_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", str(exe), os.path.join(ROOT, "tests", "sight", "sight_host_main.cpp")])
    files = []
    for world in sc.WORLDS:
        m, q = sc.model_of(world), sc.all_queries(world)
        heights = m.height_rows(1)
        files.append(tmp_path / f"{world}.sgt")
        tables_file(files[-1], m, heights, q, m.visible(q, heights))
    pair, sector, shut = sc.hand_door()
    m = sc.model_of("hand")
    q = np.repeat(pair, 3)
    q["frame"] = [0, 1, 2]
    heights = m.height_rows(3, [[], [shut], []])
    files.append(tmp_path / "door.sgt")
    tables_file(files[-1], m, heights, q, m.visible(q, heights))
    for depth in (sc.SIGHT_MAX_DEPTH - 1, sc.SIGHT_MAX_DEPTH):
        m, q = sc.model_of(f"chain{depth}"), sc.chain_queries(depth)
        assert m.depth() == depth
        heights = m.height_rows(1)
        want = m.visible(q, heights)
        assert 0 < want.sum() < len(q)
        files.append(tmp_path / f"chain{depth}.sgt")
        tables_file(files[-1], m, heights, q, want)
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "sight_host_main: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"depth {sc.SIGHT_MAX_DEPTH}, deepest stack {sc.SIGHT_MAX_DEPTH}" in r.stdout          # a whole-strip line fills a lane's column to its last entry
