"""dg_raster_tiles / dg_raster_tiles_anyw at every launch shape launch_raster can pick, and at the staging limit of strip_body
(csrc/kernels.hip).  The frame size and the batch size choose the decomposition: the kernel (width a multiple of 4 or not), the number of
64-column strips and of 64-row tile rows, the live rows of the last tile row (<= 8: the packed pass), the tile rows per workgroup
(raster_tile_rows_per_wg) and whether the workgroups of a frame are remapped onto one XCD (raster_block).  SHAPES lists one frame size per
decision; test_the_shape_table_reaches_every_launch_class restates the launcher in Python and checks that together they reach every class.

Lists: shape_case (records, columns and visplanes placed at the frame's edges, strip boundaries and tile-row boundaries, at any W x H),
test_fuzz_lists.random_case at the small sizes, dense_case (overfull strips on both sides of a strip boundary, spans crossing every
tile-row boundary: the column-group re-staging inside the tile-row loop) and the empty frame.  Expected frames come from tests/np_mappers.py.
CPU tier: oracle == numpy for every case.  GPU tier: dg_draw_lists == numpy alone, in a batch of 9 and in a batch of 24 in reversed order,
with the XCD remap forced off and on; the 512-span staging limit; full renders at the size extremes against the oracle; the byte path of
dg_frame_checksums.
"""
import hashlib

import numpy as np
import pytest

import np_mappers as nm
from test_edge_kats import to_dg_lists, view_dict, wall
from test_fuzz_lists import CASES as FUZZ_CASES, FLATS, TEXTURES, random_case

TILE = 64
SPAN_CAP = 512            # kernels.hip SPAN_CAP = binner.cpp kMaxSpansPerColumn
PACK_ROWS = 8
BATCHES = (1, 9, 24)
OPAQUE = ["BRICK1", "BRICK2", "BRICK3", "STONE2", "METAL2", "PANEL2", "WIDE2", "TALL72"]
HOLEY = ["HOLEY1", "GRATE1", "COMBO2"]

# (W, H): the launcher decisions the size is here for (n = batch size)
SHAPES = [
    (1, 1, "smallest frame: any-width kernel, one strip, one tile row with 1 live row, packed pass"),
    (2, 1, "W % 4 = 2, one live row"),
    (3, 2, "W % 4 = 3, two live rows"),
    (1, 200, "one column, 4 tile rows, last tile row has 8 live rows (packed pass), 2 tile rows per workgroup"),
    (63, 9, "one strip one column short of full, 9 live rows (one past the packed pass)"),
    (65, 65, "two strips, the last of ONE column; two tile rows, the last with 1 live row; XCD remap possible (gx = 2)"),
    (68, 127, "W % 4 = 0 with a 4-column last strip; last tile row has 63 live rows"),
    (129, 72, "three strips, the last of one column; last tile row has 8 live rows"),
    (130, 73, "W % 4 = 2, three strips; last tile row has 9 live rows"),
    (191, 513, "any-width, 9 tile rows (>= 8): 3 tile rows per workgroup, 1 live row in the last"),
    (256, 512, "W % 4 = 0, 8 tile rows: 3 + 3 + 2 tile rows per workgroup, last tile row full (64 live rows)"),
    (1283, 97, "21 strips (> 8), last strip 3 columns, any-width, 33 live rows"),
    (4096, 8, "64 strips, one tile row of 8 live rows"),
    (16384, 72, "widest frame: 256 strips, above 1.1 M pixels (XCD remap off by default)"),
    (72, 16384, "tallest frame: 256 tile rows, 86 segments of 3 with a last one of 1"),
    (16384, 1025, "17 tile rows x 256 strips: at n = 24 four tile rows per workgroup, last segment of 1"),
]


# ---- launch_raster / raster_tile_rows_per_wg / raster_block, restated --------------------------------------------------------------------

def tile_rows_per_wg(W, H, n):
    ntr = (H + TILE - 1) // TILE
    if ntr < 8:
        return min(2, ntr)
    strips = ((W + TILE - 1) // TILE) * max(1, n)
    segments = (30000 + strips - 1) // strips
    segments = max(1, min(segments, (ntr + 2) // 3))
    return (ntr + segments - 1) // segments


def launch_plan(W, H, n, frame_per_xcd=None):
    """What launch_raster does for n frames of W x H; frame_per_xcd = the DOOMGPU_FRAME_PER_XCD override (None: not set)."""
    ntr = (H + TILE - 1) // TILE
    trpw = tile_rows_per_wg(W, H, n)
    gx, gy = (W + TILE - 1) // TILE, (ntr + trpw - 1) // trpw
    pf = gx * gy
    remap = W * H <= 1100000 if frame_per_xcd is None else bool(frame_per_xcd)
    if gx < 2 or pf * n * pf >= 1 << 32:
        remap = False
    return {"anyw": W % 4 != 0, "strips": gx, "last_strip_cols": W - (gx - 1) * TILE, "tile_rows": ntr,
            "live_last": H - (ntr - 1) * TILE, "trpw": trpw, "segments": gy, "last_segment": ntr - (gy - 1) * trpw,
            "remap": remap, "remapped_frames": (n & ~7) if remap else 0, "n": n}


def launch_classes(p):
    c = {("anyw", p["anyw"])}
    c.add(("strips", "1" if p["strips"] == 1 else "2" if p["strips"] == 2 else ">8" if p["strips"] > 8 else "3-8"))
    if p["strips"] > 1 and p["last_strip_cols"] == 1:
        c.add(("last strip of 1 column",))
    c.add(("tile rows", "1" if p["tile_rows"] == 1 else "<8" if p["tile_rows"] < 8 else ">=8"))
    c.add(("live rows in last tile row", p["live_last"]))
    c.add(("tile rows per wg", p["trpw"] if p["trpw"] <= 3 else ">3"))
    if p["trpw"] >= 3 and p["last_segment"] < p["trpw"]:
        c.add(("unequal last segment", p["trpw"] if p["trpw"] <= 3 else ">3"))
    if p["remap"] and p["n"] % 8:
        c.add(("remap on, frames past the last multiple of 8",))
    if p["remap"] and p["remapped_frames"]:
        c.add(("remap on",))
    if not p["remap"]:
        c.add(("remap off",))
    return c


REQUIRED_CLASSES = {
    ("anyw", False), ("anyw", True),
    ("strips", "1"), ("strips", "2"), ("strips", ">8"), ("last strip of 1 column",),
    ("tile rows", "1"), ("tile rows", "<8"), ("tile rows", ">=8"),
    *[("live rows in last tile row", k) for k in (1, 8, 9, 63, 64)],
    ("tile rows per wg", 1), ("tile rows per wg", 2), ("tile rows per wg", 3), ("tile rows per wg", ">3"),
    ("unequal last segment", 3), ("unequal last segment", ">3"),
    ("remap on",), ("remap on, frames past the last multiple of 8",), ("remap off",),
}


def test_tile_rows_per_wg_restates_the_library(dg):
    """The restatement against the host function launch_raster calls (exported by libdoomgpu.so; pure host code, no device needed),
    at every shape of the table and a grid of sizes and batch sizes."""
    import ctypes
    fn = getattr(dg.lib(), "_ZN2dg23raster_tile_rows_per_wgEiii")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    sizes = {(W, H) for W, H, _ in SHAPES} | {(W, H) for W in (1, 63, 64, 65, 320, 1024, 2560, 16384) for H in (1, 200, 449, 511, 768, 1600, 16384)}
    for W, H in sorted(sizes):
        for n in (*BATCHES, 0, 8, 250, 1000, 65535):
            assert fn(W, H, n) == tile_rows_per_wg(W, H, n), (W, H, n)


def test_launch_plan_xcd_rule():
    assert launch_plan(1024, 768, 1000)["remap"] and not launch_plan(1920, 1080, 1000)["remap"]
    assert launch_plan(1280, 859, 9)["remap"] and not launch_plan(1280, 860, 9)["remap"]   # 1 100 000 pixels and one row more
    assert not launch_plan(64, 40, 24, frame_per_xcd=1)["remap"]               # gx < 2: one strip per frame, nothing to deal
    assert launch_plan(16384, 200, 16383, frame_per_xcd=1)["remap"]             # 512 workgroups per frame: total * pf = 2^32 - 2^18
    assert not launch_plan(16384, 200, 16384, frame_per_xcd=1)["remap"]         # = 2^32: the reciprocals would not be exact


def test_the_shape_table_reaches_every_launch_class():
    got = set()
    for W, H, _ in SHAPES:
        for n in BATCHES:
            for fpx in (None, 0, 1):
                got |= launch_classes(launch_plan(W, H, n, fpx))
    missing = REQUIRED_CLASSES - got
    assert not missing, f"no shape of SHAPES reaches {sorted(map(str, missing))}"
    # the default decision alone reaches both XCD mappings too
    dflt = set().union(*(launch_classes(launch_plan(W, H, n)) for W, H, _ in SHAPES for n in BATCHES))
    assert {("remap on",), ("remap off",), ("remap on, frames past the last multiple of 8",)} <= dflt


def test_fuzz_lists_cases_are_unchanged():
    """random_case now takes W or H = 1; the lists test_fuzz_lists draws at its own sizes are the same as before."""
    assert hashlib.sha256(repr(FUZZ_CASES).encode()).hexdigest() == "2d591e0a90c4f72f62cf39be061911dea9897742d896d52c7d034c81e871ab48"


# ---- lists for any W x H ----------------------------------------------------------------------------------------------------------------

def _focus(W, H):
    xs = {0, W - 1} | {b + d for b in range(TILE, W, TILE) for d in (-1, 0)}
    ys = {0, H - 1} | {b + d for b in range(TILE, H, TILE) for d in (-1, 0)} | {H - 1 - PACK_ROWS, H - PACK_ROWS}
    xs, ys = sorted(x for x in xs if 0 <= x < W), sorted(y for y in ys if 0 <= y < H)
    return xs, ys


def _line(rng, f):
    kind = rng.integers(0, 8)
    if kind == 0:
        sx = f(-50, 300); sy = f(-200, 200); return (sx, sy, sx, sy)
    if kind == 1:
        return (0.0, f(-30, 30), f(0.01, 50), f(-30, 30))
    if kind == 2:
        return (f(1e4, 1e6), f(-1e6, 1e6), f(1e4, 1e6), f(-1e6, 1e6))
    return (f(0.01, 600), f(-400, 400), f(0.01, 600), f(-400, 400))


def shape_case(seed, W, H):
    """Random records whose columns and visplanes sit on the frame's edges, the strip boundaries (x = 64k - 1, 64k), the tile-row
    boundaries and the packed pass's rows, with bounded extents so that the numpy frame stays cheap at 16384 columns or rows."""
    rng = np.random.default_rng(seed)
    f = lambda lo, hi: float(np.float32(rng.uniform(lo, hi)))
    xs, ys = _focus(W, H)
    pick = lambda v, n: int(v[int(rng.integers(0, len(v)))]) if rng.integers(0, 4) else int(rng.integers(0, n))   # (one in four anywhere)
    view = (f(-4000, 4000), f(-4000, 4000), f(-7, 7), float(rng.integers(-200, 200)))
    columns, renders, planes = [], [], []
    for _ in range(int(rng.integers(3, 9))):
        xc, yc = pick(xs, W), pick(ys, H)
        n = int(rng.integers(1, min(W, 40) + 1))
        x0 = xc - int(rng.integers(0, n + 2))
        cols = []
        for x in range(x0, x0 + n + 2):
            if rng.integers(0, 5) == 0:
                continue
            ct = yc - int(rng.integers(0, 24)); cb = min(H - 1, yc + int(rng.integers(0, 24)))    # (a row H panics in the reference)
            if rng.integers(0, 8) == 0:
                ct, cb = cb, ct - 1                                                              # empty: ct > cb
            style = rng.integers(0, 6)
            if style == 0:
                ty = by = int(rng.integers(-50, 90)) + yc
            elif style == 1:
                ty, by = -32768, 32767
            else:
                ty = ct - int(rng.integers(0, 120)); by = cb + int(rng.integers(0, 120))
            cols.append((x, ct, cb, max(-32768, min(32767, by)), max(-32768, min(32767, ty))))
        if not cols:
            continue
        start_x = x0 - int(rng.integers(0, 30)); end_x = x0 + n + int(rng.integers(0, 30))
        if rng.integers(0, 6) == 0:
            end_x = start_x
        tex = str(rng.choice(TEXTURES))
        renders.append(wall(tex, int(rng.integers(-60, 360)), _line(rng, f), start_x, end_x, f(-600, 200), f(-200, 600), cols, columns,
                            offset_x=int(rng.integers(-400, 400)) if rng.integers(0, 4) else int(rng.choice([-32768, 32767])),
                            offset_y=int(rng.integers(-400, 400)) if rng.integers(0, 4) else int(rng.choice([-32768, 32767])),
                            start_offset=f(-100, 1000)))
    for _ in range(int(rng.integers(1, 4))):
        xc, yc = pick(xs, W), pick(ys, H)
        left = max(0, xc - int(rng.integers(0, 20))); right = min(W - 1, left + int(rng.integers(0, 40)))
        tb = []
        for x in range(left, right + 1):
            t = yc - int(rng.integers(0, 12))
            b = t + int(rng.integers(0, 25)) if rng.integers(0, 5) else t + int(rng.integers(-2, 3))
            tb.append((t, b))
        planes.append({"flat": str(rng.choice(FLATS)), "height": int(rng.integers(-300, 300)), "light_level": int(rng.integers(-60, 360)),
                       "left": left, "right": right, "tb": tb})
    order = [(0, i) for i in range(len(renders))] + [(1, i) for i in range(len(planes))]
    order = [order[i] for i in rng.permutation(len(order))]
    return view, {"renders": renders, "columns": columns, "visplanes": planes, "order": order}


def dense_case(seed, W, H):
    """Overfull strips on both sides of up to two strip boundaries b: columns b - 2, b - 1 (strip b / 64 - 1) and b, b + 1 (strip b / 64)
    carry 250, 300, 400 and 200 spans, every strip holding more than SPAN_CAP; span i of a column crosses the boundary of tile row
    i % tile_rows, so every tile row of every workgroup segment re-stages column groups (kernels.hip strip_body, `!fits`)."""
    rng = np.random.default_rng(seed)
    ntr = (H + TILE - 1) // TILE
    bounds = [b for b in range(TILE, W - 1, TILE)]
    bounds = sorted(set([bounds[0], bounds[-1]])) if len(bounds) > 1 else bounds
    per_col = {}
    for b in bounds:
        per_col.update({b - 2: 250, b - 1: 300, b: 400, b + 1: 200})
    columns, renders = [], []
    for r in range(max(per_col.values())):
        holey = r % 5 == 3
        tex = HOLEY[r % len(HOLEY)] if holey else OPAQUE[r % len(OPAQUE)]
        cols = []
        for x, n in sorted(per_col.items()):
            if r < n:
                j = (r + x) % ntr
                ct = TILE * j - 1 - int(rng.integers(0, 6))
                cb = min(H - 1, TILE * j + int(rng.integers(0, 9)))
                cols.append((x, ct, cb, cb + int(rng.integers(0, 4)), ct - int(rng.integers(0, 4))))
        renders.append(wall(tex, 255 - (r % 200), (50.0 + (r % 97), -20.0 + (r % 13), 70.0 + (r % 89), 25.0), min(per_col) - 3, max(per_col) + 3,
                            -41.0, 87.0, cols, columns, offset_x=r % 128, offset_y=-(r % 77)))
    planes = []                                            # a floor under each group, so that uncovered rows are not black
    for b in bounds:
        left, right = b - 4, min(W - 1, b + 3)
        planes.append({"flat": "FLOOR1", "height": -16, "light_level": 160, "left": left, "right": right, "tb": [(0, H - 1)] * (right - left + 1)})
    order = [(1, i) for i in range(len(planes))] + [(0, i) for i in range(len(renders))]
    return (float(rng.integers(-300, 300)), float(rng.integers(-300, 300)), 0.4, 0.0), \
        {"renders": renders, "columns": columns, "visplanes": planes, "order": order}


EMPTY = ((0.0, 0.0, 0.0, 0.0), {"renders": [], "columns": [], "visplanes": [], "order": []})


def spans_per_column(W, H, lists):
    n = np.zeros(W, dtype=np.int64)
    for c in lists["columns"]:
        if 0 <= c[0] < W and max(c[1], 0) <= min(c[2], H - 1):
            n[c[0]] += 1
    for p in lists["visplanes"]:
        n[p["left"]:p["right"] + 1] += 1                   # an upper bound (a plane column of 0 or 1 row may be skipped)
    return n


def cases_for(W, H):
    """[(name, view, lists)] drawn at W x H."""
    k = SHAPES.index(next(s for s in SHAPES if s[:2] == (W, H)))
    out = [(f"shape{i}", *shape_case(8000 + 10 * k + i, W, H)) for i in range(2)]
    if W * H <= 130 * 73:
        out.append(("random", *random_case(9000 + k, W, H)))
    if W > TILE + 1 and H > 7 * TILE:
        out.append(("dense", *dense_case(9500 + k, W, H)))
    out.append(("empty", *EMPTY))
    return out


CASES = {(W, H): cases_for(W, H) for W, H, _ in SHAPES}


def test_dense_cases_reach_the_restaging_paths():
    """A strip other than the first holds more than SPAN_CAP spans, at >= 3 tile rows per workgroup, in both kernels."""
    reached = set()
    for (W, H), cases in CASES.items():
        for name, _, lists in cases:
            if name != "dense":
                continue
            n = spans_per_column(W, H, lists)
            assert n.max() <= SPAN_CAP
            over = [s for s in range((W + TILE - 1) // TILE) if n[s * TILE:(s + 1) * TILE].sum() > SPAN_CAP]
            assert over and over[-1] > 0
            for nb in BATCHES:
                p = launch_plan(W, H, nb)
                if p["trpw"] >= 3:
                    reached.add(("anyw", p["anyw"]))
                    if p["last_segment"] < p["trpw"]:
                        reached.add(("unequal",))
    assert reached == {("anyw", True), ("anyw", False), ("unequal",)}


@pytest.fixture(scope="module")
def np_wad(wad1993):
    return nm.Wad(wad1993)


_EXPECTED = {}


def expected_frames(campath_mod, np_wad, W, H):
    """[(name, rec, lists, numpy frame)] for the cases at W x H (memoised: the CPU and GPU tiers share them within a run)."""
    if (W, H) not in _EXPECTED:
        out = []
        for name, view, lists in CASES[(W, H)]:
            rec, vd = view_dict(campath_mod, *view)
            out.append((name, rec, lists, nm.draw_lists(np_wad, "SKY1", W, H, vd, lists)))
        _EXPECTED[(W, H)] = out
    return _EXPECTED[(W, H)]


def _diff(got, want, label):
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert len(bad) == 0, f"{label}: {len(bad)} pixels differ, first at (x={bad[0][1]}, y={bad[0][0]}): got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("W,H", [s[:2] for s in SHAPES], ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_oracle_equals_independent_restatement_at_every_shape(oracle_scene1993, campath_mod, np_wad, W, H):
    drawn = 0
    for name, rec, lists, want in expected_frames(campath_mod, np_wad, W, H):
        got = np.frombuffer(oracle_scene1993.draw_lists(W, H, rec, lists), dtype=np.uint8).reshape(H, W, 3)
        _diff(got, want, f"{W}x{H} {name}")
        if name == "empty":
            assert not want.any()
        drawn += int(want.any(axis=2).sum())
    assert drawn > 0


# ---- the 512-span staging limit ---------------------------------------------------------------------------------------------------------

STAGE_W, STAGE_H = 130, 73


def column_stack(spans):
    """{x: n}: n wall spans on column x (record r has one column on every x with r < n), short spans walking down the frame and over
    the tile-row boundary, over a floor plane that puts one more span on every column."""
    columns, renders = [], []
    for r in range(max(spans.values())):
        cols = [(x, (3 * r + x) % (STAGE_H - 4), (3 * r + x) % (STAGE_H - 4) + 1 + r % 4, (3 * r + x) % (STAGE_H - 4) + 6, (3 * r + x) % (STAGE_H - 4) - 2)
                for x, n in sorted(spans.items()) if r < n]
        tex = HOLEY[r % len(HOLEY)] if r % 7 == 3 else OPAQUE[r % len(OPAQUE)]
        renders.append(wall(tex, 255 - (r % 190), (60.0 + (r % 50), -15.0, 75.0 + (r % 40), 18.0), 60, 110, -41.0, 87.0, cols, columns,
                            offset_x=r % 64, offset_y=r % 31))
    planes = [{"flat": "FLOOR3", "height": -8, "light_level": 200, "left": 0, "right": STAGE_W - 1, "tb": [(0, STAGE_H - 1)] * STAGE_W}]
    return {"renders": renders, "columns": columns, "visplanes": planes, "order": [(1, 0)] + [(0, i) for i in range(len(renders))]}


STAGE_VIEW = (-100.0, 300.0, 0.4, 0.0)
STAGE_CASES = {
    "strip_of_512": {5: SPAN_CAP - TILE},                 # + 64 plane spans: the first strip holds exactly SPAN_CAP, staged at once
    "column_of_512": {64: SPAN_CAP - 1, 100: 3},          # + the plane span: second strip, the 512 column is a group of its own (c_hi = c_lo + 1)
    "two_columns_of_512": {64: SPAN_CAP - 1, 65: SPAN_CAP - 1},   # two groups of exactly 512, one after the other
}


def test_stage_cases_hold_what_they_claim():
    n = spans_per_column(STAGE_W, STAGE_H, column_stack(STAGE_CASES["strip_of_512"]))
    assert n[:TILE].sum() == SPAN_CAP
    for name in ("column_of_512", "two_columns_of_512"):
        n = spans_per_column(STAGE_W, STAGE_H, column_stack(STAGE_CASES[name]))
        assert n[64] == SPAN_CAP and n.max() == SPAN_CAP and n[TILE:2 * TILE].sum() > SPAN_CAP, name
    assert spans_per_column(STAGE_W, STAGE_H, column_stack(STAGE_CASES["two_columns_of_512"]))[65] == SPAN_CAP
    n = spans_per_column(STAGE_W, STAGE_H, column_stack({64: SPAN_CAP}))
    assert n[64] == SPAN_CAP + 1                         # the one refused: 513


@pytest.fixture(scope="module")
def stage_expected(campath_mod, np_wad):
    rec, vd = view_dict(campath_mod, *STAGE_VIEW)
    return rec, {name: nm.draw_lists(np_wad, "SKY1", STAGE_W, STAGE_H, vd, column_stack(s)) for name, s in STAGE_CASES.items()}


def test_oracle_equals_independent_restatement_at_the_staging_limit(oracle_scene1993, stage_expected):
    rec, want = stage_expected
    for name, spans in STAGE_CASES.items():
        got = np.frombuffer(oracle_scene1993.draw_lists(STAGE_W, STAGE_H, rec, column_stack(spans)), dtype=np.uint8).reshape(STAGE_H, STAGE_W, 3)
        _diff(got, want[name], name)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------

BIG = 16 * 1024 * 1024       # frames of more bytes are compared by device checksum, not read back


def _batches(cases):
    """alone / 9 / 24 reversed, as lists of case indices.  Batch 24 (drawn first) puts a drawn frame in every slot, batch 9 then draws
    the empty frame into slot 0; the densest case sits next to sparse ones in both."""
    empty = next(i for i, c in enumerate(cases) if c[0] == "empty")
    drawn = [i for i in range(len(cases)) if i != empty]
    densest = max(drawn, key=lambda i: len(cases[i][2]["columns"]))
    seq24 = [drawn[k % len(drawn)] for k in range(24)]
    seq24[5] = empty
    seq24[11] = densest
    b24 = seq24[::-1]
    assert b24[0] != empty
    b9 = [empty] + [drawn[k % len(drawn)] for k in range(8)]
    b9[4] = densest
    return [("batch24_reversed", b24), ("batch9", b9)] + [(f"alone_{cases[i][0]}", [i]) for i in range(len(cases))]


@pytest.mark.gpu
@pytest.mark.parametrize("fpx", ["0", "1"], ids=["xcd_remap_off", "xcd_remap_on"])
@pytest.mark.parametrize("W,H", [s[:2] for s in SHAPES], ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_gpu_draws_every_shape_alike_in_any_batch(dg, wad1993, campath_mod, np_wad, monkeypatch, W, H, fpx):
    exp = expected_frames(campath_mod, np_wad, W, H)
    monkeypatch.setenv("DOOMGPU_FRAME_PER_XCD", fpx)                          # read by every raster launch
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=24, slots=1)
    ctx.upload_scene(scene)
    try:
        lists = [to_dg_lists(dg, scene, rec, l) for _, rec, l, _ in exp]
        sums = [dg.frame_checksum(want) for *_, want in exp] if 3 * W * H > BIG else None
        for label, idx in _batches(exp):
            frames = (dg.DgFrameLists * len(idx))(*[lists[i][0] for i in idx])
            if sums is None:
                out = ctx.draw_lists(0, frames)
                for k, i in enumerate(idx):
                    _diff(out[k], exp[i][3], f"{W}x{H} {label} frame {k} ({exp[i][0]})")
            else:
                dg._check(dg.lib().dg_draw_lists(ctx._h, 0, frames, len(idx), None))     # (no read-back)
                got = ctx.frame_checksums(0, 0, len(idx))
                bad = [(k, exp[i][0]) for k, i in enumerate(idx) if int(got[k]) != sums[i]]
                assert not bad, f"{W}x{H} {label}: frames {bad} differ from numpy (device checksum)"
    finally:
        ctx.close()
        scene.close()


@pytest.mark.gpu
def test_gpu_staging_limit(dg, wad1993, stage_expected):
    """Columns of exactly SPAN_CAP spans render like numpy; a column of 513 is refused before any launch with DG_ERR_CAPACITY, and the
    ctx draws correctly right after."""
    rec, want = stage_expected
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(STAGE_W, STAGE_H, max_batch=4, slots=1)                   # list slab: 4 x 130 x 24 spans, far above 513
    ctx.upload_scene(scene)
    try:
        for name, spans in STAGE_CASES.items():
            fl, keep = to_dg_lists(dg, scene, rec, column_stack(spans))
            out = ctx.draw_lists(0, (dg.DgFrameLists * 2)(fl, fl))
            for k in range(2):
                _diff(out[k], want[name], f"{name} frame {k}")
        fl, keep = to_dg_lists(dg, scene, rec, column_stack({64: SPAN_CAP}))
        with pytest.raises(dg.DoomGpuError) as ei:
            ctx.draw_lists(0, (dg.DgFrameLists * 1)(fl))
        assert ei.value.code == dg.DG_ERR_CAPACITY and "512 spans" in str(ei.value)
        fl, keep = to_dg_lists(dg, scene, rec, column_stack(STAGE_CASES["two_columns_of_512"]))
        _diff(ctx.draw_lists(0, (dg.DgFrameLists * 1)(fl))[0], want["two_columns_of_512"], "after the refusal")
    finally:
        ctx.close()
        scene.close()


EXTREME_SIZES = [(1, 1), (1, 200), (2, 1), (320, 1), (3, 3), (63, 9), (16384, 72), (72, 16384)]
FRONT_ENDS = (1, 2, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("front_end", FRONT_ENDS, ids=["host-lists", "device-column-walk", "device-seg-walk"])
@pytest.mark.parametrize("seed", [1993, 1994])
def test_gpu_full_renders_at_size_extremes(dg, wad1993, wad1994, oracle_scene1993, oracle_scene1994, path1993, path1994, seed, front_end):
    wad, osc, path = (wad1993, oracle_scene1993, path1993) if seed == 1993 else (wad1994, oracle_scene1994, path1994)
    scene = dg.Scene(wad, "e1m1")
    try:
        for W, H in EXTREME_SIZES:
            idx = [0, 297, 623, 900] if W * H < 100000 else [623]
            ctx = dg.Context(W, H, max_batch=len(idx), slots=1, front_end=front_end)
            ctx.upload_scene(scene)
            out = ctx.render(dg.make_views(path[idx]))
            for k, i in enumerate(idx):
                ref = np.frombuffer(osc.render(W, H, path[i]), dtype=np.uint8).reshape(H, W, 3)
                _diff(out[k], ref, f"map {seed} {W}x{H} path frame {i} front end {front_end}")
            ctx.close()
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_largest_frame_by_checksum(dg, wad1993, oracle_scene1993, path1993):
    """One 16384 x 16384 view (805 MB of RGB24) through DG_FE_AUTO, compared by device checksum with the oracle's frame."""
    W = H = 16384
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=1, slots=1)
    ctx.upload_scene(scene)
    try:
        ctx.submit(0, dg.make_views(path1993[[623]]))
        ctx.wait(0)
        got = int(ctx.frame_checksums(0, 0, 1)[0])
    finally:
        ctx.close()
        scene.close()
    ref = np.frombuffer(oracle_scene1993.render(W, H, path1993[623]), dtype=np.uint8)
    assert ref.any()
    assert got == checksum_in_chunks(ref)


def checksum_in_chunks(rgb24, chunk=1 << 24):
    """frame_checksum for a frame of a multiple of 4 bytes, a chunk of dwords at a time (the sum wraps mod 2^64 either way)."""
    d = rgb24.view("<u4")
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for i0 in range(0, d.size, chunk):
            i = np.arange(i0, min(d.size, i0 + chunk), dtype=np.uint64)
            m = (d[i0:i0 + chunk].astype(np.uint64) ^ (i * np.uint64(0x9E3779B97F4A7C15))) * np.uint64(0xBF58476D1CE4E5B9)
            total += (m ^ (m >> np.uint64(32))).sum(dtype=np.uint64)
    return int(total)


def test_checksum_in_chunks_is_frame_checksum(dg):
    raw = np.random.default_rng(5).integers(0, 256, size=3 * 40 * 20, dtype=np.uint8)
    assert checksum_in_chunks(raw, chunk=97) == checksum_in_chunks(raw) == dg.frame_checksum(raw)


CHECKSUM_SIZES = [(7, 1), (1, 2), (3, 3), (131, 67)]     # 3 W H = 1, 2, 3, 3 mod 4
CHECKSUM_SEEDS = range(9200, 9205)


def test_checksum_cases_draw(campath_mod, np_wad):
    """The frames the byte-path test checksums are not all black past frame 0 (path views leave a 1-column frame black)."""
    for W, H in CHECKSUM_SIZES:
        assert (3 * W * H) % 4 != 0
        drawn = []
        for seed in CHECKSUM_SEEDS:
            view, lists = random_case(seed, W, H)
            rec, vd = view_dict(campath_mod, *view)
            drawn.append(nm.draw_lists(np_wad, "SKY1", W, H, vd, lists).any())
        assert any(drawn[1:]) and any(drawn[3:]), (W, H, drawn)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", CHECKSUM_SIZES)
def test_gpu_checksum_byte_path(dg, wad1993, campath_mod, W, H):
    """Frames that end in a partial dword and (first > 0) do not start on one: dg_frame_checksums == frame_checksum of the frames read back."""
    scene = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=len(CHECKSUM_SEEDS), slots=1)
    ctx.upload_scene(scene)
    try:
        keep = [to_dg_lists(dg, scene, view_dict(campath_mod, *v)[0], l) for v, l in (random_case(s, W, H) for s in CHECKSUM_SEEDS)]
        out = ctx.draw_lists(0, (dg.DgFrameLists * len(keep))(*[k[0] for k in keep]))
        for first, count in ((1, 4), (3, 1), (4, 1), (0, 5)):
            got = ctx.frame_checksums(0, first, count)
            want = [dg.frame_checksum(out[first + k]) for k in range(count)]
            assert [int(v) for v in got] == want, f"{W}x{H} frames {first}..{first + count - 1}"
    finally:
        ctx.close()
        scene.close()
