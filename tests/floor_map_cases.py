"""The views and parameters of the floor-textured map frames' tests, CPU and GPU tier alike (test_floor_map_host.py,
test_floor_map_gpu.py), on three worlds:

  light     synth:1993 with the light effects' test sectors (light_fx.fx_wad), DG_LIGHT_THINKERS on with seed SEED
  hand      the hand-assembled IWAD of test_hand_wad.py: room A (sector 0, FLOORA) and room B (sector 1, NUKAGE1: animated)
  hand_sky  the same with room A's floor flat replaced by F_SKY1 — neither map above has a sky floor, so this file builds one

A case names a world, a view (x, y, angle; trig_valid = 0), a timestamp, scale and flags, a mask recipe and the view's light and flat
entries.  Importing this module asserts, from the numpy model alone (np_floor_map at 64x48), that over the cases every pixel class
occurs: floor, background by geometry, sky floor, a sector the mask hides, a line, the arrow, an animated flat that differs between
two timestamps, a light entry and a flat entry that change floor pixels.

Further down, each with its own assertions at import: WITNESS_CASES (pixel centres at which the side test is 0.0 and a fused one is not),
TIE_CASES (centres exactly on the partition, on segs and on vertices), CORNER_CASES (the contract's corners) and wave_shapes (which
waves of dg_floor_map_tiles the cases produce).
"""
import copy
import functools
import math

import numpy as np

import light_fx as lf
import np_automap as na
import np_ego as ng
import np_floor_map as nf
from test_hand_wad import build_hand_iwad

SEED = 7
R, A = ng.ROTATE, ng.ARROW
EXTRA_FLATS = {"light": ["FLOOR3", "FLOOR4", "F_SKY1"], "hand": ["CEILA", "NUKAGE2"], "hand_sky": []}     # names the cases' flat entries use (Scene.use_flat before an upload)


def _hand_sky() -> bytes:
    lumps = lf._lumps(build_hand_iwad())
    i = next(k for k, (n, _) in enumerate(lumps) if n == "SECTORS")
    b = lumps[i][1]
    assert b[4:12] == b"FLOORA\0\0"
    lumps[i] = ("SECTORS", b[:4] + b"F_SKY1\0\0" + b[12:])
    return lf._pack(lumps)


@functools.lru_cache(maxsize=None)
def wad_of(world: str) -> bytes:
    return {"light": lf.fx_wad, "hand": build_hand_iwad, "hand_sky": _hand_sky}[world]()


@functools.lru_cache(maxsize=None)
def model_of(world: str) -> nf.FloorModel:
    return nf.FloorModel(wad_of(world))


def case(name, world, x, y, angle, ts, scale, flags, mask=None, lights=(), flats=()):
    return dict(name=name, world=world, view=(float(np.float32(x)), float(np.float32(y)), float(np.float32(angle))), ts=float(np.float32(ts)), scale=scale, flags=flags,
                mask=mask, lights=tuple(lights), flats=tuple(flats))


def _sector_at(world, x, y) -> int:
    m = model_of(world)
    leaf = m.leaf_at(np.array([np.float32(x)]), np.array([np.float32(y)]))
    return int(m.leaf_sector[leaf[0]])


# positions on synth:1993's camera path (tests/golden/campath_seed1993.f32, records 0, 297, 623): inside the level
P0, P1, P2 = (256.0, 256.0, -0.7853982), (283.31277, 2289.3289, 3.1241908), (2814.2759, 478.53192, -1.6973493)


def _cases():
    out = []
    for k, (x, y, a) in enumerate((P0, P1, P2)):
        out.append(case(f"light_whole_{k}", "light", x, y, a, 0.4 * k, 0.05, (R | A) if k % 2 else 0))
        out.append(case(f"light_unit_{k}", "light", x, y, a, 1.0 + k, 1.0, A if k % 2 else R))
    out.append(case("light_close", "light", *P1, 2.0, 16.0, R | A))
    out.append(case("light_masked_half", "light", *P0, 0.0, 0.05, R | A, mask=("half", 3)))
    out.append(case("light_masked_zero", "light", *P2, 0.0, 0.05, A, mask=("zero",)))
    out.append(case("light_masked_ones", "light", *P2, 0.0, 0.05, A, mask=("ones",)))
    s0, s1 = _sector_at("light", P0[0], P0[1]), _sector_at("light", P1[0], P1[1])
    assert s0 >= 0 and s1 >= 0
    out.append(case("light_entries", "light", *P0, 0.7, 1.0, R, lights=[(s0, 255), (s1, 96), (s0, 40)], flats=[(s0, "FLOOR4" if model_of("light").sectors[s0][0] == "FLOOR3" else "FLOOR3")]))
    out.append(case("light_entries_base", "light", *P0, 0.7, 1.0, R))
    out.append(case("light_flat_to_sky", "light", *P1, 0.0, 1.0, 0, flats=[(s1, "F_SKY1")]))
    for ts in (0.0, 0.4, 0.7):
        out.append(case(f"hand_animated_{ts}", "hand", 600.0, 250.0, math.pi - 0.2, ts, 0.25, R | A))
    out.append(case("hand_whole", "hand", 352.5, 250.0, 0.1, 0.0, 0.05, A))
    out.append(case("hand_room_a_only", "hand", 352.5, 250.0, 0.1, 0.4, 0.1, R, mask=("lines", (0, 1, 2))))
    out.append(case("hand_entries", "hand", 96.0, 180.0, 0.35, 0.4, 0.5, R | A, lights=[(0, 80), (1, 300)], flats=[(0, "CEILA"), (1, "NUKAGE2")]))
    out.append(case("hand_close", "hand", 300.0, 140.0, 1.2, 0.0, 16.0, 0))
    out.append(case("sky_floor", "hand_sky", 352.5, 250.0, 0.1, 0.0, 0.1, R | A))
    out.append(case("sky_floor_masked", "hand_sky", 96.0, 180.0, 0.0, 0.4, 0.25, 0, mask=("lines", (6,))))
    out.append(case("light_whole_rotated", "light", *P0, 0.0, 0.05, R))                    # (ROTATION_WITNESS below)
    out.append(case("light_long_wall", "light", *_long_wall_view(), 0.0, 0.0, 0.5, 0))     # (wave_shapes below)
    return out


def _long_wall_view(W: int = 131, H: int = 67, row: int = 20):
    """(x, y) from which, unrotated at scale 0.5, a horizontal linedef of the light world longer than the frame is wide crosses a whole
    row of a WxH frame: row 20 of 131x67 ends at band pixel 2750, so its line covers wave 41 (pixels 2624 .. 2687) and lanes 0 .. 62 of
    wave 42 — wave_shapes says what comes of it."""
    e = model_of("light").ego
    for v1, v2, fl in e.lines:
        (x1, y1), (x2, y2) = e.verts[v1], e.verts[v2]
        if y1 == y2 and abs(x2 - x1) >= 2 * W + 16 and not fl & 128:
            return float(x1 + x2) / 2.0, float(y1) - 2.0 * (H // 2 - row) + 1.0                       # Y = H / 2 - (y - view.y) * 0.5 lands in the row
    raise AssertionError("the light world has no horizontal linedef that long")


def mask_row(c, row: int = 0):
    """The case's mask row (uint32 words), or None.  row: a batch's frames take different random halves."""
    if c["mask"] is None:
        return None
    m = model_of(c["world"]).ego
    ones = m.bits_to_row(range(m.n_lines))
    kind = c["mask"][0]
    if kind == "half":
        return np.random.default_rng(c["mask"][1] + 101 * row).integers(0, 1 << 32, m.words, dtype=np.uint64).astype(np.uint32) & ones
    if kind == "lines":
        return m.bits_to_row(c["mask"][1])
    return ones if kind == "ones" else np.zeros(m.words, np.uint32)


def lights_of(c, ts=None):
    """The sectors' levels before the view's entries: the light effects' at the timestamp in the world that has them on."""
    return lf.levels_at(wad_of(c["world"]), SEED, c["ts"] if ts is None else ts) if c["world"] == "light" else None


def model_frame(c, W: int, H: int, row: int = 0, classes: bool = False):
    m = model_of(c["world"])
    f, cls = m.frame_classes(W, H, na.libm_view(*c["view"]), c["ts"], c["scale"], c["flags"], mask_row(c, row), lights_of(c), c["lights"], c["flats"])
    return (f, cls) if classes else f


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- the product's side of a case -------------------------------------------------------------------------------------------------

def open_scene(dg, world: str):
    """The world's scene with its effects on and the cases' extra flats loaded: ready to upload."""
    sc = dg.Scene(wad_of(world), "e1m1")
    if world == "light":
        sc.set_light_effects(dg.DG_LIGHT_THINKERS, SEED)
    for name in EXTRA_FLATS[world]:
        sc.use_flat(name)
    return sc


def view_of(dg, c):
    x, y, a = c["view"]
    return dg.DgView(x, y, a, 0, 0, 0, 0, 0, c["ts"], 0)


def state_of(c):
    """(lights, mobjs) as make_view_states takes it, or None."""
    return (list(c["lights"]), []) if c["lights"] else None


def surfaces_of(sc, c):
    """(sides, flats) as make_view_surfaces takes it, or None: the floor handle from the name, the ceiling's as loaded."""
    if not c["flats"]:
        return None
    loaded = sc.sector_flats()
    return ([], [(s, sc.use_flat(name), int(loaded[s][2])) for s, name in c["flats"]])


# ---- what the cases show, from the model alone --------------------------------------------------------------------------------------

def _covered():
    W, H = 64, 48
    seen = set()
    frames = {}
    for c in CASES:
        f, cls = model_frame(c, W, H, classes=True)
        frames[c["name"]] = (f, cls)
        seen |= set(np.unique(cls).tolist())
    missing = {n for n, v in (("floor", nf.FLOOR), ("line", nf.LINE), ("arrow", nf.ARROW), ("sky floor", nf.SKY), ("hidden by the mask", nf.HIDDEN)) if v not in seen}
    if not seen & {nf.NO_SECTOR, nf.BEHIND}:
        missing.add("background by geometry")
    floor = lambda n: frames[n][1] == nf.FLOOR
    both = floor("hand_animated_0.0") & floor("hand_animated_0.4")
    if not (frames["hand_animated_0.0"][0][both] != frames["hand_animated_0.4"][0][both]).any():
        missing.add("an animated flat at two timestamps")
    c = BY_NAME["light_entries"]
    m = model_of("light")
    args = (W, H, na.libm_view(*c["view"]), c["ts"], c["scale"], c["flags"], None, lights_of(c))
    base = m.frame(*args)
    if not (m.frame(*args, c["lights"], ()) != base).any():
        missing.add("a light entry")
    if not (m.frame(*args, (), c["flats"]) != base).any():
        missing.add("a flat entry")
    assert not missing, f"floor_map_cases shows no pixel of: {sorted(missing)}"


_covered()


# ---- points on the lines: witnesses of a fused side test, exact ties, the contract's corners ------------------------------------------
# The side tests (walk_left_of, floor_behind) are sums of two products that must not fuse.  On the maps above no pixel centre comes
# within a rounding of a diagonal line, so a fused test would draw the same frames.  These views put pixel centres there.
F = np.float32
SIDE, BEHIND_TEST, ROTATION = nf.SIDE, nf.BEHIND_TEST, nf.ROTATION
HAND_WALLS = ("lines", (0, 1, 2, 3, 4, 5))                # without the portal's linedef (6), which would draw over the points on it
HAND_TWO = ("lines", (1, 4))                              # one wall of each room: both floors show, most lines do not
SIZES = ((131, 67), (320, 200))


def fused_model(world: str, *places) -> nf.FloorModel:
    """The world's model with the named sums of two products fused (np_floor_map.sum2)."""
    m = copy.copy(model_of(world))
    m.fused = frozenset(places)
    return m


def fused_frame(c, W: int, H: int, *places, classes: bool = False):
    m = fused_model(c["world"], *places)
    f, cls = m.frame_classes(W, H, na.libm_view(*c["view"]), c["ts"], c["scale"], c["flags"], mask_row(c), lights_of(c), c["lights"], c["flats"])
    return (f, cls) if classes else f


def pixel_view(mx, my, k: int, j: int, scale):
    """(view.x, view.y) of the unrotated view whose pixel (W / 2 + k, H / 2 - j) has its centre at (mx, my), in every frame size: the
    rule's r = (k + 0.5) / scale and f = (j - 0.5) / scale added back without a rounding."""
    inv = F(F(1.0) / F(scale))
    r, f = (F(k) + F(0.5)) * inv, (F(j) - F(0.5)) * inv
    x, y = F(F(mx) - r), F(F(my) - f)
    assert F(x + r) == F(mx) and F(y + f) == F(my), (mx, my, k, j, scale)
    return float(x), float(y)


def witness_point(t: int):
    """A point of the hand world's partition (origin (384, 96), direction (-64, 304)) at which the rule's test is 0.0 and a fused one is
    not: bx = -64 makes ay * bx exact, so with ay = -fl(ax * 304) / 64 both rounded products are equal, while the exact ax * 304 is off
    by its rounding error.  ax = -33 + t * 2^-15: ax * 304 = -10032 + t * 9.5 ulp, so an odd t is a tie of the rounding, and of those
    t = 3, 7, 11 .. round so that the exact test is positive: "right" for a fused descent.  The points 1/16 to the left and 19/64 up, and
    so on along the line, are witnesses as well.  (_witnesses asserts what the frames show.)"""
    mx = F(351.0) + F(t) * F(2.0 ** -15)
    ax = F(mx - F(384.0))
    my = F(F(96.0) - F(ax * F(304.0)) / F(64.0))
    return mx, my


def _witness_cases():
    out = []
    for t in (3, 7, 11):
        x, y = pixel_view(*witness_point(t), 0, -30, 64.0)      # 30 rows below the centre: at 131x67 four pixels of the line are in the frame
        out.append(case(f"witness_{t}", "hand", x, y, 0.0, 0.0, 64.0, 0, mask=HAND_WALLS))
    return out


def _tie_cases():
    return [case("tie_scale_1", "hand", *pixel_view(394.0, 104.0, 0, 0, 1.0), 0.0, 0.0, 1.0, 0, mask=HAND_TWO),      # about p1 (384, 96): whole coordinates
            case("tie_scale_2", "hand", *pixel_view(325.0, 394.0, 0, 0, 2.0), 0.0, 0.4, 2.0, 0, mask=HAND_TWO),      # about p2 (320, 400): halves
            case("tie_scale_64", "hand", *pixel_view(364.0, 191.0, 3, -20, 64.0), 0.0, 0.0, 64.0, 0, mask=HAND_TWO)]  # on the portal: 64ths


def _corner_cases():
    """The contract's corners (ego_check_call, ego_check_view), one frame each; a case carries its frame size."""
    far = 2.0 ** -10
    return [dict(case("corner_scale_min", "light", 2048.0, 1536.0, P1[2], 0.0, far, R | A), size=(320, 200)),
            dict(case("corner_scale_max", "light", *P1, 0.7, 64.0, R | A), size=(320, 200)),
            dict(case("corner_view_65536", "light", 65536.0, -65536.0, 0.3, 0.0, far, A), size=(320, 200)),
            dict(case("corner_view_minus_65536", "light", -65536.0, 65536.0, 0.3, 0.0, far, R), size=(320, 200)),
            dict(case("corner_wide", "light", 65536.0, 1536.0, 0.0, 0.0, far, 0), size=(16384, 16))]                # the wide tile: |mx| up to 2^23 + 2^16, where floorf is the identity


WITNESS_CASES, TIE_CASES, CORNER_CASES = _witness_cases(), _tie_cases(), _corner_cases()
ROTATION_WITNESS = BY_NAME["light_whole_rotated"]


def _free(*classes):
    """The pixels no line or arrow covers in any of the class planes."""
    out = np.ones(classes[0].shape, bool)
    for cls in classes:
        out &= ~np.isin(cls, (nf.LINE, nf.ARROW))
    return out


def side_witness_points():
    """(xs, ys): the pixel centres of the witness frames at 320x200 that the rule puts in room A (sector 0, floor 0) and a fused
    walk_left_of in room B (sector 1, floor 24) — the walks' starts and the poses' entries of the other two tiers."""
    xs, ys = [], []
    for c in WITNESS_CASES:
        m = model_of("hand")
        mx, my = m.map_points(320, 200, na.libm_view(*c["view"]), c["scale"], False)
        a, b = m.leaf_at(mx, my), fused_model("hand", SIDE).leaf_at(mx, my)
        xs.append(mx[a != b]); ys.append(my[a != b])
        assert (a[a != b] == 0).all() and (b[a != b] == 1).all()
    return np.concatenate(xs), np.concatenate(ys)


def _cross(mx, my, x1, y1, x2, y2):
    """The rule's (mx - x1) * (y2 - y1) - (my - y1) * (x2 - x1), unfused."""
    return nf.sum2(mx - F(x1), F(F(y2) - F(y1)), my - F(y1), F(F(x2) - F(x1)), -1, False)


def tie_counts(c, W: int, H: int):
    """Of the pixels no line covers: how many centres lie exactly on the hand world's partition (the test is 0.0), on a one-sided seg of
    their own leaf between its ends, and on a vertex."""
    m = model_of(c["world"])
    _, cls = model_frame(c, W, H, classes=True)
    free = _free(cls)
    mx, my = m.map_points(W, H, na.libm_view(*c["view"]), c["scale"], bool(c["flags"] & R))
    leaf = m.leaf_at(mx, my)
    (nx, ny, ndx, ndy), = m.node_line
    on_partition = free & (_cross(mx, my, nx, ny, nx + ndx, ny + ndy) == 0.0)
    on_seg = np.zeros(mx.shape, bool)
    for l, (first, count) in enumerate(m.leaves):
        for v1, v2, ld, _ in m.segs[first:first + count]:
            if min(m.line_sides[ld]) >= 0:
                continue
            x1, y1, x2, y2 = m.vx[v1], m.vy[v1], m.vx[v2], m.vy[v2]
            between = (mx >= min(x1, x2)) & (mx <= max(x1, x2)) & (my >= min(y1, y2)) & (my <= max(y1, y2))
            on_seg |= free & (leaf == l) & between & (_cross(mx, my, x1, y1, x2, y2) == 0.0)
    on_vertex = free & ((mx[..., None] == m.vx) & (my[..., None] == m.vy)).any(axis=2)
    return dict(partition=int(on_partition.sum()), seg=int(on_seg.sum()), vertex=int(on_vertex.sum()))


def tie_points():
    """(xs, ys): the tie frames' pixel centres at 131x67 that lie exactly on the partition, a one-sided seg or a vertex, lines or not."""
    m = model_of("hand")
    xs, ys = [], []
    for c in TIE_CASES:
        mx, my = m.map_points(131, 67, na.libm_view(*c["view"]), c["scale"], False)
        on = np.zeros(mx.shape, bool)
        for v1, v2, _, _ in m.segs:
            on |= _cross(mx, my, m.vx[v1], m.vy[v1], m.vx[v2], m.vy[v2]) == 0.0
        xs.append(mx[on]); ys.append(my[on])
    return np.concatenate(xs), np.concatenate(ys)


def _witnesses():
    """What the views above show, from the model alone."""
    for c in WITNESS_CASES:
        for W, H in SIZES:
            f, cls = model_frame(c, W, H, classes=True)
            for places, (was, now) in (((SIDE,), (nf.FLOOR, nf.FLOOR)), ((BEHIND_TEST,), (nf.FLOOR, nf.BEHIND)), ((SIDE, BEHIND_TEST), (nf.FLOOR, nf.FLOOR))):
                g, gcls = fused_frame(c, W, H, *places, classes=True)
                d = (f != g).any(axis=2) & _free(cls, gcls)
                assert d.sum() >= 4, (c["name"], W, H, places, int(d.sum()))
                # both signs: a fused descent says "right" (room B's floor) where the rule says "left"; a fused seg test says "behind"
                # (background) where the rule says "inside"
                assert (cls[d] == was).all() and (gcls[d] == now).all(), (c["name"], W, H, places)
    xs, ys = side_witness_points()
    assert len(xs) >= 24, len(xs)
    c = ROTATION_WITNESS
    assert c["flags"] & R
    d = (model_frame(c, 320, 200) != fused_frame(c, 320, 200, ROTATION)).any(axis=2)
    assert d.sum() >= 16, int(d.sum())
    seen = dict(partition=0, seg=0, vertex=0)
    for c in TIE_CASES:
        n = tie_counts(c, 131, 67)
        assert n["partition"] >= 1, (c["name"], n)
        for k in seen:
            seen[k] += n[k]
    assert seen["seg"] >= 1 and seen["vertex"] >= 1, seen
    assert {c["scale"] for c in TIE_CASES} == {1.0, 2.0, 64.0}


_witnesses()


# ---- the shapes of dg_floor_map_tiles' waves ------------------------------------------------------------------------------------------
# The kernel walks a band's pixels (ego_band_rows rows of the frame, row-major) in trips of 256, a wave of 64 neighbours at a time; a lane
# wants a floor where no line or arrow lies.  The wanting lanes descend together while they take the same child and part where they
# do not (floor_lane).  wave_shapes names what occurs in a frame, cut from the model's classes as the kernel cuts.
WAVE_SHAPES = ("no wanting lane", "lanes 0..31 under lines, a later one wants", "only lane 63 wants", "a partial last wave",
               "a whole wave past the band's pixels", "parts at the root", "parts at the last node above its leaves, below the root",
               "one leaf for the wave")


def _children(m, mx, my):
    """Per level of the descent the child each point takes (bit 15: a leaf), -1 below its leaf: (levels, n) int64."""
    n_nodes = len(m.node_line)
    cur = np.full(mx.shape, n_nodes - 1, np.int64)
    live = np.ones(mx.shape, bool)
    levels = []
    with np.errstate(all="ignore"):
        while live.any():
            n = m.node_line[np.where(live, cur, 0)]
            left = _cross(mx, my, n[:, 0], n[:, 1], n[:, 0] + n[:, 2], n[:, 1] + n[:, 3]) <= F(0.0)
            child = np.where(live, m.node_child[np.where(live, cur, 0), np.where(left, 1, 0)], -1)
            levels.append(child)
            live &= (child & 0x8000) == 0
            cur = np.where(live, child, cur)
    return np.stack(levels)


def wave_shapes(c, W: int, H: int):
    m = model_of(c["world"])
    _, cls = model_frame(c, W, H, classes=True)
    want_all = _free(cls).ravel()
    mx, my = m.map_points(W, H, na.libm_view(*c["view"]), c["scale"], bool(c["flags"] & R))
    child = _children(m, mx.ravel(), my.ravel())
    rows = 1 if W >= 8192 else 8192 // W
    seen = set()
    for row0 in range(0, H, rows):
        px = min(rows, H - row0) * W
        for lo in range(0, -(-px // 256) * 256, 64):
            if lo >= px:
                seen.add(WAVE_SHAPES[4])
                continue
            if lo + 64 > px:
                seen.add(WAVE_SHAPES[3])
            at = row0 * W + np.arange(lo, min(lo + 64, px))
            want = want_all[at]
            if not want.any():
                seen.add(WAVE_SHAPES[0])
                continue
            if not want[:32].any():
                seen.add(WAVE_SHAPES[1])
            if want.sum() == 1 and len(want) == 64 and want[63]:
                seen.add(WAVE_SHAPES[2])
            for level, ch in enumerate(child[:, at[want]]):
                if (ch != ch[0]).any():
                    if level == 0:
                        seen.add(WAVE_SHAPES[5])
                    elif ((ch & 0x8000) != 0).all():
                        seen.add(WAVE_SHAPES[6])
                    break
                if ch[0] & 0x8000:
                    seen.add(WAVE_SHAPES[7])
                    break
    return seen


WAVE_CASES = ("light_long_wall", "light_whole_0", "light_whole_2", "hand_whole")      # at 131x67, where both tiers run every case


def _wave_shapes_covered():
    seen = set()
    for name in WAVE_CASES:
        seen |= wave_shapes(BY_NAME[name], 131, 67)
    assert seen == set(WAVE_SHAPES), sorted(set(WAVE_SHAPES) - seen)
    assert {WAVE_SHAPES[k] for k in (0, 1, 2)} <= wave_shapes(BY_NAME["light_long_wall"], 131, 67)


_wave_shapes_covered()
