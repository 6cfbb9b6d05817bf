"""The host walker's failure paths (csrc/frontend.cpp Walker, both modes): views in which the reference would panic before or inside its
column loops.  Four edits of the hand-packed IWAD of tests/test_hand_wad.py, seen from its player start at 64x40:

    (a) texture     a one-sided wall in view whose middle texture is in no TEXTURE lump          Textures::get panics (textures.rs:158)
    (b) lower       the portal's lower texture, seen from the low room, is in no TEXTURE lump    the same, in the third call of the seg
    (c) flat        the floor flat of the sector in view has no lump                             Flat::new unwrap (flats.rs:117)
    (d) zero-sized  the barrel's picture is 20 x 0 / 0 x 30 (the loader admits both)             the reference divides by zero when it draws

For each: the return code and dg_last_error text of dg_build_lists (list mode), the return code and text of build_frame_parts (parts mode,
through tests/emul), and, where dg_build_lists succeeds, what the binner (the host half of dg_draw_lists, through tests/emul: a Context needs
a device) says of the lists.  The literals are what the walker gave before list mode took its geometry from fs_core.h; list mode and parts
mode must name the same failure for the same view.  A wall TEXTURE of non-positive size never reaches the walker: the loader refuses the WAD."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hand_wad as hw

W, H = 64, 40
PARTS_UNSUPPORTED = 1000                                       # csrc/frontend.hpp kPartsUnsupported
TEXTURE = "Unknown texture (Textures::get panics, textures.rs:158)"
FLAT = "Could not find flat lump (Flat::new unwrap, flats.rs:117)"


def _lump(wad: bytes, name: str):
    n, diro = struct.unpack_from("<II", wad, 4)
    for i in range(n):
        off, size = struct.unpack_from("<II", wad, diro + 16 * i)
        if wad[diro + 16 * i + 8: diro + 16 * i + 16] == hw._name8(name):
            return off, size
    raise KeyError(name)


def _poke(wad: bytes, lump: str, at: int, data: bytes) -> bytes:
    off, size = _lump(wad, lump)
    assert at + len(data) <= size
    return wad[:off + at] + data + wad[off + at + len(data):]


def _barrel(w: int, h: int) -> bytes:
    """The hand WAD with another picture for the barrel (BAR1A0): a lump of another length, so the WAD is packed again."""
    wad = hw.build_hand_iwad()
    n, diro = struct.unpack_from("<II", wad, 4)
    lumps = []
    for i in range(n):
        off, size = struct.unpack_from("<II", wad, diro + 16 * i)
        name = wad[diro + 16 * i + 8: diro + 16 * i + 16]
        lumps.append((name, hw._picture(w, h, 10, 28, lambda x, y: 7) if name == hw._name8("BAR1A0") else wad[off:off + size]))
    body, directory = b"", b""
    for (name, data) in lumps:
        directory += struct.pack("<II", 12 + len(body), len(data)) + name
        body += data
    return b"IWAD" + struct.pack("<II", len(lumps), 12 + len(body)) + body + directory


def _wads():
    base = hw.build_hand_iwad()
    # sidedef i (30 B): xoff, yoff, upper[8] at +4, lower[8] at +12, middle[8] at +20, sector; sector j (26 B): floor flat[8] at +4
    return {
        "texture": _poke(base, "SIDEDEFS", 30 * 0 + 20, hw._name8("NOSUCH")),     # sidedef 0: the wall p1 -> a0 of room A
        "lower": _poke(base, "SIDEDEFS", 30 * 7 + 12, hw._name8("NOSUCH")),       # sidedef 7: the portal's side in room A (B's floor is 24 higher)
        "flat": _poke(base, "SECTORS", 26 * 0 + 4, hw._name8("NOFLAT")),          # sector 0: room A
        "zero-height": _barrel(20, 0),
        "zero-width": _barrel(0, 30),
    }


# case -> (dg_build_lists rc, its text, build_frame_parts rc, its text, the binner's rc and text where the lists were built)
ZERO = "zero-sized bitmap"
EXPECT = {
    "texture": (-5, TEXTURE, -5, TEXTURE, None),
    "lower": (-5, TEXTURE, -5, TEXTURE, None),
    "flat": (-5, FLAT, -5, FLAT, None),
    "zero-height": (0, "", PARTS_UNSUPPORTED, ZERO, (-5, "zero-sized bitmap (reference divides by zero)")),
    "zero-width": (0, "", PARTS_UNSUPPORTED, ZERO, (0, "")),
}


@pytest.fixture(scope="module")
def start_view(campath_mod):
    return campath_mod.view_record(np.float32(96.0), np.float32(180.0), np.float32(0.0), np.float32(0.0))   # the player start, room A's floor


@pytest.mark.parametrize("case", list(EXPECT))
def test_both_walker_modes_name_the_same_failure(dg, start_view, case):
    import emul_bind
    wad = _wads()[case]
    lists_rc, lists_text, parts_rc, parts_text, binner = EXPECT[case]
    assert dg.DG_ERR_RENDER == -5
    scene = dg.Scene(wad, "e1m1")
    view = dg.make_views(start_view[None, :])[0]
    fl = dg.DgFrameLists()
    rc = dg.lib().dg_build_lists(scene._h, W, H, ctypes.byref(view), ctypes.byref(fl))
    text = dg.lib().dg_last_error().decode() if rc else ""
    es = emul_bind.EmulScene(wad)
    prc, ptext = es.build_parts(W, H, start_view)
    print(case, "lists:", rc, repr(text), "parts:", prc, repr(ptext))
    got_binner = None
    if rc == 0:
        assert fl.n_renders > 0 and fl.n_columns > 0 and fl.n_order > 0
        buf = np.empty(3 * W * H, dtype=np.uint8)
        st = (ctypes.c_uint64 * 4)()
        brc = emul_bind.lib().emul_draw_lists(es._h, W, H, ctypes.byref(fl), buf.ctypes.data_as(ctypes.c_void_p), st)
        got_binner = (brc, emul_bind.lib().emul_last_error().decode() if brc else "")
        print(case, "binner:", got_binner)
    assert (rc, text) == (lists_rc, lists_text)
    assert (prc, ptext) == (parts_rc, parts_text)
    assert got_binner == binner
    if lists_rc and parts_rc != PARTS_UNSUPPORTED:
        assert (rc, text) == (prc, ptext)                       # the same view, the same failure, whichever mode walked it


def test_the_loader_refuses_a_wall_texture_of_no_size(dg):
    """TEXTURE1's WALLA as 0 x 128: csrc/scene.cpp turns the WAD away (Texture::load would allocate nothing and index it), so a zero-sized
    wall bitmap cannot reach the walker through a WAD — only a zero-sized sprite picture can."""
    base = hw.build_hand_iwad()
    off, _ = _lump(base, "TEXTURE1")
    first = struct.unpack_from("<I", base, off + 4)[0]
    assert base[off + first: off + first + 8] == hw._name8("WALLA")
    wad = _poke(base, "TEXTURE1", first + 12, struct.pack("<h", 0))
    with pytest.raises(dg.DoomGpuError) as e:
        dg.Scene(wad, "e1m1")
    assert e.value.code == dg.DG_ERR_WAD and "non-positive size" in str(e.value)
