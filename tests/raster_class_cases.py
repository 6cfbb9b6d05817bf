"""Hand-built draw lists aimed at the span classes and chunk paths of dg_raster_tiles (tests/test_raster_classes.py), in the list-dict form of
test_edge_kats.build_cases.  Every boundary value is computed here in numpy.float32 from the class condition it sits on; none is typed in.

Two frame sizes hold every kind of tile between them:
  72x136  strip 0 = 64 columns, strip 1 = 8 columns (columns 64..71: every wave of that strip has ONE live column); tile row 0 (rows 0..63)
          has no horizon row, tile row 1 holds row 68 where vy == 0, tile row 2 has 8 live rows: the packed pass;
  72x137  CFY = 68.5: no vy == 0 row anywhere, |vy| = 0.5 next to the horizon; tile row 2 has 9 live rows, one past the packed pass.

A case is (name, view, lists, notes); `notes` says what the case was built for, in terms the coverage table of the test checks through the
observer (emul_bind.EmulScene.observe_lists):
  notes["groups"]    [(label, intended reason, [render indices])]: float32 neighbours on both sides of one class boundary — some of the
                     renders must come out plain, the others not plain for exactly the intended reason
  notes["mixes"]     [(path, tile row, [columns])]: the pixels of these columns in that tile row take that path and hold every class of MIX_CLASSES
  notes["overlays"]  [(path, tile row, [columns], "after" | "before")]: a possibly-transparent span drawn after / before the opaque owner
  notes["light_bands"] {light level: [columns]}, notes["wz"]: the planes of the light cases

The lower edge of the prepared divide's guard band (|numerator| = 2^-64, raster_core.h div_guard_ok) is not reachable through dg_draw_lists:
wz = height as f32 - floor_height - 41.0 (visplanes.rs:112) with an integer height, so a non-zero wz is at least one ulp of an operand of
magnitude >= 1 after the first subtraction that does not cancel exactly, or a difference of two f32 near 41 — never below 2^-24 x 41 in
magnitude unless floor_height itself is tiny, and then wz is an integer minus 41; GCFX = 43.2 and a non-zero |vx| >= 1 / ARC = 1.2 cannot
scale that down to 2^-64.  wz == 0 exactly (numerators +-0, inside the band by definition) is covered instead.
"""
import numpy as np

from test_edge_kats import wall

f32 = np.float32
SIZES = [(72, 136), (72, 137)]
TEX_H = {"BRICK1": 128, "BRICK3": 128, "STONE2": 128, "TALL72": 72, "HOLEY1": 128, "GRATE1": 128, "COMBO2": 128}   # checked against the WAD by the test
HOLEY = ("HOLEY1", "GRATE1", "COMBO2")
LINE = (100.0, -30.0, 180.0, 50.0)
LIGHTS = [-32768, 1784, 1785, 2041, 2042, 32767]      # lightf < 7 ends at 1785; from 2042 a texel at saturated distance is no longer black
MIX_CLASSES = {"none", "sky", "plain_flat", "light7", "plain_wall", "npot", "first_out"}
PILE = 9                                              # spans under a column that make it a column of more than 8 spans


def tile_rows(H):
    return [(y0, min(y0 + 63, H - 1)) for y0 in range(0, H, 64)]


def frame_consts(W, H):
    arc = f32(200.0) / f32(240.0)
    return {"ARC": arc, "GCFX": f32(W) / arc / f32(2.0), "CFX": f32(W) / f32(2.0), "CFY": f32(H) / f32(2.0)}


# ---- the class conditions restated in float32 (resolve_wall_span / resolve_flat_span, raster_core.h) ---------------------------------

def wall_reasons(h, ctop, cbot, top_y, bottom_y, uy1):
    """-> set of reason names of a wall span (empty = plain)."""
    out = set()
    if h & (h - 1):
        out.add("npot")
    d = f32(bottom_y - top_y)
    if d == 0:
        out.add("d0")
        return out
    with np.errstate(all="ignore"):
        for name, y in (("first_out", ctop), ("last_out", cbot)):
            v = f32(h) + (f32(y - top_y) / d) * f32(uy1)
            if not abs(v) < f32(32000.0):
                out.add(name)
    return out


def guard_ok(n):
    """div_guard_ok: zero, or a biased exponent in [63, 191] — 2^-64 <= |n| < 2^65 (the exponent test lets the whole binade of 2^64 in)."""
    bits = int(np.array(n, dtype=np.float32).view(np.uint32))
    e = (bits >> 23) & 0xFF
    return (bits & 0x7FFFFFFF) == 0 or 63 <= e <= 191


def flat_reasons(W, H, x, height, floor_height, light):
    k = frame_consts(W, H)
    out = set()
    with np.errstate(all="ignore"):
        wz = f32(height) - f32(floor_height) - f32(41.0)
        if not guard_ok(k["GCFX"] * wz):
            out.add("gwz_out")
        if not guard_ok(wz * ((k["CFX"] - f32(x)) / k["ARC"])):
            out.add("wzvx_out")
        if not f32(light) / f32(255.0) < f32(7.0):
            out.add("light7")
    return out


# ---- builder ----------------------------------------------------------------------------------------------------------------------------

class Lists:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.columns, self.renders, self.planes, self.order = [], [], [], []
        self.notes = {"groups": [], "mixes": [], "overlays": []}

    def wall(self, texture, cols, uy1, light=200, offset_y=0, offset_x=0):
        """One render record (bottom_height 0, top_height uy1: uy1 = top - bottom is then that f32 exactly) -> its index."""
        self.renders.append(wall(texture, light, LINE, 0, self.W - 1, 0.0, float(f32(uy1)), list(cols), self.columns, offset_x=offset_x, offset_y=offset_y))
        self.order.append((0, len(self.renders) - 1))
        return len(self.renders) - 1

    def plane(self, flat, height, light, left, right, tb):
        self.planes.append({"flat": flat, "height": height, "light_level": light, "left": left, "right": right, "tb": list(tb)})
        self.order.append((1, len(self.planes) - 1))
        return len(self.planes) - 1

    def pile(self, xs):
        """PILE one-row spans at the top of each of these columns, drawn first: a column of more than 8 spans in EVERY tile row."""
        self.wall("BRICK3", [(x, 0, 0, 10, -10) for x in xs for _ in range(PILE)], 128.0)

    def lists(self):
        return {"renders": self.renders, "columns": self.columns, "visplanes": self.planes, "order": self.order}


def edge_uy1(h, edge, k):
    """uy1 with h + k * uy1 == edge as nearly as float32 has it, and its two float32 neighbours."""
    u = (f32(edge) - f32(h)) / f32(k)
    return [np.nextafter(u, f32(-np.inf)), u, np.nextafter(u, f32(np.inf))]


def walls_case(W, H, texture, piled):
    """Every wall class condition in every tile row, two columns per configuration.  Per tile row (rows r0..r1, n of them), with d = +-1 so
    that ay is the integer k = (y - top_y) / d:
      |h + k uy1| on both sides of 32000 at the first row only (|k| = n there, 1 on the last row) and at the last row only, for d = +1 and
        d = -1, for +32000 and -32000, uy1 = (edge - h) / k and its two neighbours;
      rows that cross +32767 / -32768 (h + k uy1 = h +- 48000 on the first row), with offset_y 0, 30000 and -32768: the i16 add wraps;
      d == 0 (bottom_y == top_y), offset_y 0 and 30000;
      columns 64..71: one span over the whole column that is plain when the bitmap height is a power of two.
    A holey texture makes every one of these a possibly-transparent span; a plain floor lies under them then."""
    L = Lists(W, H)
    h = TEX_H[texture]
    if piled:
        L.pile(range(W))
    if texture in HOLEY:
        L.plane("FLOOR1", 0, 200, 0, W - 1, [(0, H - 1)] * W)
    x = 0
    for sign in (1, -1):
        for end in ("first_out", "last_out"):
            for d in (1, -1):
                group = []
                for c in range(3):
                    for (r0, r1) in tile_rows(H):
                        n = r1 - r0 + 1
                        top_y = r1 + 1 if end == "first_out" else r0 - 1
                        k = (r0 - top_y if end == "first_out" else r1 - top_y) * d          # ay on the row that carries the edge
                        group.append(L.wall(texture, [(x + j, r0, r1, top_y + d, top_y) for j in range(2)], edge_uy1(h, sign * 32000.0, k)[c]))
                        assert abs(k) == n
                    x += 2
                L.notes["groups"].append((f"{'+' if sign > 0 else '-'}32000 {end} d={d}", end, group))
    for sign in (1, -1):
        for off_y in (0, 30000, -32768):
            for (r0, r1) in tile_rows(H):
                n = r1 - r0 + 1
                L.wall(texture, [(x + j, r0, r1, r1 + 2, r1 + 1) for j in range(2)], f32(-sign * 48000.0) / f32(n), offset_y=off_y)
            x += 2
    for off_y in (0, 30000):
        for (r0, r1) in tile_rows(H):
            L.wall(texture, [(x + j, r0, r1, r0 + 3, r0 + 3) for j in range(2)], 100.0, offset_y=off_y)
        x += 2
    assert x == 64
    L.wall(texture, [(xx, 0, H - 1, H + 20, -20) for xx in range(64, W)], 128.0, offset_y=-7)
    return L


def lights_case(W, H, wz_sign):
    """Six planes side by side, one per light level of LIGHTS, each over whole columns: the rows run into the horizon from both sides, so
    wx crosses +32767 (saturated distance) on the side where wz and vy have the same sign and is <= -32768 on the other, where the factor
    saturates bright and the texel stays visible.  wz = +-2000.  Columns with x % 12 >= 8 left of column 64 are piled."""
    L = Lists(W, H)
    L.pile([x for x in range(64) if x % 12 >= 8])
    bands = {}
    for i, light in enumerate(LIGHTS):
        L.plane("FLOOR0", 41 + 2000 * wz_sign, light, 12 * i, 12 * i + 11, [(0, H - 1)] * 12)
        bands[light] = list(range(12 * i, 12 * i + 12))
    L.notes["light_bands"] = bands
    L.notes["wz"] = 2000.0 * wz_sign
    return L


def guard_floor_heights(W, H):
    """-> [(name, view floor_height)]: wz = 0 - floor_height - 41 puts GCFX * wz (and wz * vx, the same product in column 0) on both sides
    of 2^64 and of 2^65 — div_guard_ok tests the exponent, so the band ends below 2^65 — from powers of two and nextafter; then far outside,
    the non-finite values bin_frame does not refuse, and wz == 0 exactly."""
    gcfx = frame_consts(W, H)["GCFX"]
    out = []
    for p in (64, 65):
        t = f32(2.0) ** f32(p) / gcfx                       # |wz| with GCFX * wz next to 2^p
        lo, hi = t, t
        while (gcfx * lo) >= f32(2.0) ** f32(p):            # the largest wz whose product stays below 2^p, the smallest that reaches it
            lo = np.nextafter(lo, f32(0))
        while (gcfx * hi) < f32(2.0) ** f32(p):
            hi = np.nextafter(hi, f32(np.inf))
        out += [(f"below_2^{p}", float(lo)), (f"at_2^{p}", float(hi))]
    out.append(("neg_at_2^65", -out[-1][1]))
    out.append(("wide_out", float(f32(2.0) ** f32(70))))
    out += [("3e38", 3e38), ("neg_3e38", -3e38), ("inf", float("inf")), ("neg_inf", float("-inf")), ("nan", float("nan")), ("wz_zero", -41.0)]
    return out


def guard_case(W, H):
    """One floor over the whole frame (height 0, light 200); columns 36..63 are piled.  The view's floor_height decides the class."""
    L = Lists(W, H)
    L.pile(range(36, 64))
    L.plane("FLOOR1", 0, 200, 0, W - 1, [(0, H - 1)] * W)
    return L


def mix_case(W, H, piled, tiles):
    """Tile rows `tiles` (of 0 and 1): every column holds, in 8-row bands from the tile's first row on, nothing, sky, a plain flat, a complex
    flat (light 2000), a plain wall, a TALL72 wall, a wall whose first row leaves the range, nothing — six spans, so that an unpiled column
    stays at 8 spans or fewer with those of the last tile row.  Last tile row: the same classes spread over the columns, class
    (x // 8) % 8 — the eight columns of a wave (x = wave + 8 k) hold one each; the plain wall of class 4 has a holey span drawn BEFORE it,
    which must not keep the tile off the packed pass."""
    L = Lists(W, H)
    if piled:
        L.pile(range(W))
    rows = tile_rows(H)
    for t in tiles:
        b = rows[t][0]
        L.plane("F_SKY1", 128, 255, 0, W - 1, [(b + 8, b + 15)] * W)
        L.plane("FLOOR1", 0, 180, 0, W - 1, [(b + 16, b + 23)] * W)
        L.plane("CEIL2", 120, 2000, 0, W - 1, [(b + 24, b + 31)] * W)
        L.wall("BRICK1", [(x, b + 32, b + 39, b + 44, b + 27) for x in range(W)], 128.0)
        L.wall("TALL72", [(x, b + 40, b + 47, b + 52, b + 35) for x in range(W)], 72.0, offset_y=5)
        L.wall("STONE2", [(x, b + 48, b + 55, b + 57, b + 56) for x in range(W)], -6000.0)
    (r0, r1) = rows[2]
    cls = lambda k: [x for x in range(64) if (x // 8) % 8 == k]
    L.plane("F_SKY1", 128, 255, 8, 15, [(r0, r1)] * 8)
    L.plane("FLOOR1", 0, 180, 16, 23, [(r0, r1)] * 8)
    L.plane("CEIL2", 120, 2000, 24, 31, [(r0, r1)] * 8)
    L.wall("HOLEY1", [(x, r0, r1, r1 + 5, r0 - 5) for x in cls(4)], 128.0)
    L.wall("BRICK1", [(x, r0, r1, r1 + 5, r0 - 5) for x in cls(4)], 128.0)
    L.wall("TALL72", [(x, r0, r1, r1 + 5, r0 - 5) for x in cls(5)], 72.0, offset_y=5)
    L.wall("STONE2", [(x, r0, r1, r1 + 2, r1 + 1) for x in cls(6)], f32(-48000.0) / f32(r1 - r0 + 1))
    L.wall("BRICK3", [(x, r0, r1, r1 + 9, r0 - 9) for x in cls(7)], 128.0, light=120)
    L.notes["mixes"] += [("BIG" if piled else "WALK", t, [x]) for t in tiles for x in range(W)]
    if piled:
        L.notes["mixes"] += [("BIG", 2, list(range(64)))]
    elif r1 - r0 + 1 <= 8:
        L.notes["mixes"] += [("PACKED", 2, [w + 8 * k for k in range(8)]) for w in range(8)]
    return L


def overlays_case(W, H):
    """A holey span drawn before and one drawn after the opaque owner, 8 columns per path, in tile row 0:
      0..7  SOLE_WALL after    8..15 SOLE_WALL before   16..23 SOLE_FLAT after   24..31 SOLE_FLAT before
      32..39 WALK after        40..47 WALK before        48..55 BIG after         56..63 BIG before
    and in the last tile row, columns 64..71: a plain wall with a holey span AFTER it — with 8 live rows that forces the tile off the
    packed pass."""
    L = Lists(W, H)
    L.pile(range(48, 64))
    after = lambda x: (x // 8) % 2 == 0
    holey = lambda xs, tex: L.wall(tex, [(x, 6, 58, 70, -6) for x in xs], 128.0, offset_y=3)
    holey([x for x in range(64) if not after(x)], "HOLEY1")
    L.wall("BRICK1", [(x, 0, 63, 80, -16) for x in range(0, 16)], 128.0)                                   # sole plain wall
    L.plane("FLOOR1", 0, 200, 16, 31, [(0, 63)] * 16)                                                    # sole plain flat
    L.wall("BRICK1", [(x, 0, 31, 40, -8) for x in range(32, 64)], 128.0)                                   # two owners: the walk
    L.wall("STONE2", [(x, 32, 63, 70, 25) for x in range(32, 64)], 128.0)
    holey([x for x in range(64) if after(x)], "GRATE1")
    for i, path in enumerate(("SOLE_WALL", "SOLE_FLAT", "WALK", "BIG")):
        L.notes["overlays"] += [(path, 0, list(range(16 * i, 16 * i + 8)), "after"), (path, 0, list(range(16 * i + 8, 16 * i + 16)), "before")]
    (r0, r1) = tile_rows(H)[2]
    L.wall("BRICK1", [(x, r0, r1, r1 + 5, r0 - 5) for x in range(64, W)], 128.0)
    L.wall("COMBO2", [(x, r0, r1, r1 + 5, r0 - 5) for x in range(64, W)], 128.0, offset_x=-17)
    L.notes["overlays"].append(("SOLE_WALL", 2, list(range(64, W)), "after"))
    return L


def build_cases(W, H):
    """-> [(name, view (x, y, angle, floor_height), lists, notes)]"""
    cases = []
    add = lambda name, view, L: cases.append((name, view, L.lists(), L.notes))
    full = (W, H) == SIZES[0]
    for texture, piled in [("BRICK1", False), ("HOLEY1", False)] + ([("TALL72", False), ("GRATE1", False), ("COMBO2", False), ("BRICK1", True), ("TALL72", True)] if full else []):
        add(f"walls_{texture}{'_piled' if piled else ''}", (0.0, 0.0, -2.1, 0.0), walls_case(W, H, texture, piled))
    for s in (1, -1):
        add(f"lights_wz{'+' if s > 0 else '-'}2000", (1000.3, -740.8, 0.7, 0.0), lights_case(W, H, s))
    for name, fh in guard_floor_heights(W, H):
        if full or name in ("below_2^65", "at_2^65", "wide_out", "neg_3e38", "inf", "nan", "wz_zero"):
            add(f"guard_{name}", (-512.0, 2048.5, 3.9, fh), guard_case(W, H))
    add("mix", (0.0, 0.0, 1.3, 16.0), mix_case(W, H, False, (0,)))
    add("mix_horizon", (0.0, 0.0, 1.3, 16.0), mix_case(W, H, False, (1,)))
    add("mix_piled", (0.0, 0.0, 1.3, 16.0), mix_case(W, H, True, (0, 1)))
    add("overlays", (10.0, 20.0, 0.4, 0.0), overlays_case(W, H))
    return cases


CASES = {size: build_cases(*size) for size in SIZES}
