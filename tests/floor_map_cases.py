"""The views and parameters of the floor-textured map frames' tests, CPU and GPU tier alike (test_floor_map_host.py,
test_floor_map_gpu.py), on three worlds:

  light     synth:1993 with the light effects' test sectors (light_fx.fx_wad), DG_LIGHT_THINKERS on with seed SEED
  hand      the hand-assembled IWAD of test_hand_wad.py: room A (sector 0, FLOORA) and room B (sector 1, NUKAGE1: animated)
  hand_sky  the same with room A's floor flat replaced by F_SKY1 — neither map above has a sky floor, so this file builds one

A case names a world, a view (x, y, angle; trig_valid = 0), a timestamp, scale and flags, a mask recipe and the view's light and flat
entries.  Importing this module asserts, from the numpy model alone (np_floor_map at 64x48), that over the cases every pixel class
occurs: floor, background by geometry, sky floor, a sector the mask hides, a line, the arrow, an animated flat that differs between
two timestamps, a light entry and a flat entry that change floor pixels.
"""
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
    return out


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
