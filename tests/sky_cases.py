"""Skies other than the opaque 256x128 SKY1 every other WAD of the suite carries, shared by tests/test_sky_holes_host.py and
tests/test_plane_shapes_gpu.py.

draw_sky (src/renderer/visplanes.rs:42-80) writes a pixel only where the sky texel is Some: a sky bitmap with transparent texels lets
whatever was drawn before show through, so the sky span is no longer "opaque from its first row to its last" and has to be evaluated in
draw order (raster_core.h resolve_sky_span's immediate flag, kernels.hip overlay_loop, the sky arms of depth_span_writes
and label_span_writes).  A sky smaller than 256x128 is indexed outside by the reference (a panic); the product never draws one: its
binner refuses a sky plane of such a bitmap (DG_ERR_RENDER), and both device front ends hand a frame with sky to that host path.  So
resolve_sky_span's `valid`, sky_row's -1 and sky_texel_offset's ~0 cannot be reached from any entry point, and the two small variants
below serve to pin the refusal: no model, oracle or reference binary is run on them.

  VARIANTS          the hand-packed IWAD of test_hand_wad.py with another sky:
                      holey        256x128, one patch: a checker of 8x8 blocks, transparent columns tx 100..103, transparent rows ty 60..61
                      holey-gap    256x128 made of 64-wide patches of the same texels that leave tx 128..191 uncovered (holes from texture
                                   composition, textures.rs:74-103, not only from picture posts)
                      small        opaque 128x64
                      small-holey  128x64 with the holes of `holey`
  sky_lists         hand-built lists on the hand WAD's textures: sky planes over an earlier wall, an earlier flat and nothing, a masked wall
                    drawn after the sky, a second sky plane over that
  synth_holey_wad   a synthetic map whose four SKY1 patches got the same holes: the WAD is built, then the lumps are replaced
"""
import struct

import numpy as np

import np_mappers as nm
from test_edge_kats import wall
from test_hand_wad import _picture, build_hand_iwad, sky_texel

def is_hole(x, y):
    return 100 <= x <= 103 or 60 <= y <= 61 or (x // 8 + y // 8) % 2 == 0


def holey_texel(x, y):
    return None if is_hole(x, y) else sky_texel(x, y)


def _shifted(ox):
    return lambda x, y: holey_texel(x + ox, y)


SKIES = {
    "holey": ({"PSKY": (256, 128, holey_texel)}, (256, 128, [(0, 0, "PSKY")])),
    "holey-gap": ({"PSKY%d" % i: (64, 128, _shifted(64 * i)) for i in (0, 1, 3)}, (256, 128, [(64 * i, 0, "PSKY%d" % i) for i in (0, 1, 3)])),
    "small": ({"PSKY": (128, 64, sky_texel)}, (128, 64, [(0, 0, "PSKY")])),
    "small-holey": ({"PSKY": (128, 64, holey_texel)}, (128, 64, [(0, 0, "PSKY")])),
}
VARIANTS = list(SKIES)
SMALL = ("small", "small-holey")               # the reference would index outside these and the product refuses them: nothing is rendered
HOLEY = ("holey", "holey-gap", "small-holey")
_wads = {}


def variant_wad(name: str) -> bytes:
    if name not in _wads:
        _wads[name] = build_hand_iwad(SKIES[name])
    return _wads[name]


# ---- hand-built lists -----------------------------------------------------------------------------------------------------------------

SKY_VIEW = (200.0, 150.0, 0.7, 0.0)            # x, y, angle, floor height
T_WALL, T_FLAT, T_SKY, T_MASKED, T_SKY2 = range(5)      # positions in the order list


def sky_lists(W, H):
    """Left third: an opaque wall; middle third: a floor plane; right third: nothing.  Then a sky plane over the upper three quarters of
    all of them, a masked wall (MASKED: 8x8 holes) across the middle rows drawn after the sky, and a second sky plane over the lower
    right, which covers part of the masked wall."""
    m, w3 = H // 2, max(1, W // 3)
    columns = []
    renders = [wall("WALLA", 176, (100.0, -30.0, 180.0, 50.0), 0, w3 - 1, -41.0, 87.0, [(x, 0, min(H - 1, m + 3 + x % 3), H, -3) for x in range(w3)], columns),
               wall("MASKED", 224, (60.0, 10.0, 90.0, -20.0), 0, W - 1, -10.0, 62.0, [(x, max(0, m - 5), min(H - 1, m + 5), m + 7, m - 7) for x in range(W)], columns,
                    offset_x=9, offset_y=-3)]
    r2 = min(W - 1, 2 * w3 - 1)
    planes = [{"flat": "FLOORA", "height": 0, "light_level": 200, "left": w3, "right": r2, "tb": [(0, H - 1)] * (r2 - w3 + 1)},
              {"flat": "F_SKY1", "height": 128, "light_level": 255, "left": 0, "right": W - 1, "tb": [(-2, min(H - 1, (3 * H) // 4 + x % 4)) for x in range(W)]},
              {"flat": "F_SKY1", "height": 128, "light_level": 255, "left": W // 2, "right": W - 1, "tb": [(m + x % 2, H + 3) for x in range(W // 2, W)]}]
    return {"renders": renders, "columns": columns, "visplanes": planes, "order": [(0, 0), (1, 0), (1, 1), (0, 1), (1, 2)]}


def sky_cover(W, H, lists, plane):
    """The pixels draw_sky visits for one sky plane of the lists (its columns' rows clamped to the frame)."""
    p = lists["visplanes"][plane]
    cover = np.zeros((H, W), dtype=bool)
    for i, x in enumerate(range(p["left"], p["right"] + 1)):
        t, b = max(p["tb"][i][0], 0), min(p["tb"][i][1], H - 1)
        if 0 <= x < W and t <= b:
            cover[t:b + 1, x] = True
    return cover


# ---- a synthetic map with a holey sky ---------------------------------------------------------------------------------------------------

def replace_lumps(wad: bytes, new: dict) -> bytes:
    """The WAD with the lumps named in `new` replaced (every entry of that name), everything else as it was, in the same order."""
    n, diro = struct.unpack_from("<ii", wad, 4)
    body, directory, hit = b"", b"", set()
    for i in range(n):
        off, size = struct.unpack_from("<ii", wad, diro + 16 * i)
        raw = wad[diro + 16 * i + 8:diro + 16 * i + 16]
        name = raw.rstrip(b"\0").decode("ascii").upper()
        data = new[name] if name in new else wad[off:off + size]
        hit |= {name} & set(new)
        directory += struct.pack("<ii", 12 + len(body), len(data)) + raw
        body += data
    assert hit == set(new), set(new) - hit
    return wad[:4] + struct.pack("<ii", n, 12 + len(body)) + body + directory


def synth_holey_wad(wad: bytes) -> bytes:
    """The four 64x128 patches of the synthetic maps' SKY1 (PSKY0 .. PSKY3 at x = 0, 64, 128, 192) with the holes of `holey`."""
    w = nm.Wad(wad)
    new = {}
    for i in range(4):
        name = "PSKY%d" % i
        pw, ph, px = w.picture(name)
        assert (pw, ph) == (64, 128) and all(t is not None for row in px for t in row)
        _w, _h, left, top = struct.unpack_from("<hhhh", w.lump(name), 0)
        new[name] = _picture(pw, ph, left, top, lambda x, y, px=px, i=i: None if is_hole(x + 64 * i, y) else px[y][x])
    return replace_lumps(wad, new)
