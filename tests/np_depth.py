"""np_depth.py — the model of the depth / surface-kind frame (include/doomgpu.h: dg_depth_*), obtained by DRIVING tests/np_mappers.py.

Test infrastructure.  np_mappers is not edited: its three mappers run as they are, with
  * diminish_color patched to return, instead of a colour, the i16 distance it was handed (two bytes) and a tag that says which mapper
    called it (render_vertical_bitmap_line: 1, draw_visplane: 2 — the two are wrapped so that the tag is known);
  * a Wad whose palette() returns the sky sentinel for every entry, so that draw_sky's direct `palette[texel]` write decodes to
    (32767, 3).
Frame.px then holds the two planes.  Overwrite order, transparency, clamps and the column rules are np_mappers' own and share nothing
with csrc/plane_core.h.  `Tracker` is a Frame that also records who wrote each pixel last.
"""
import contextlib
import struct
from unittest import mock

import numpy as np

import np_mappers as nm

FAR = 32767
SKY_SENTINEL = (FAR & 255, FAR >> 8, 3)


class DepthWad(nm.Wad):
    """np_mappers.Wad with every palette entry replaced by the sky sentinel (nothing else reads the palette once diminish_color is patched)."""

    def palette(self):
        return [SKY_SENTINEL] * 256


class Tracker(nm.Frame):
    """A Frame that records, per pixel, the tag (`current`) of the draw call that wrote it last; -1 = never written."""
    made = []

    def __init__(self, W, H):
        super().__init__(W, H)
        self.writer = np.full((H, W), -1, dtype=np.int64)
        self.current = 0
        Tracker.made.append(self)

    def set(self, x, y, rgb):
        if 0 <= x < self.W and 0 <= y < self.H:
            self.writer[y, x] = self.current
        super().set(x, y, rgb)


@contextlib.contextmanager
def depth_mappers():
    """np_mappers with diminish_color returning (distance lo, distance hi, mapper tag)."""
    state = {"kind": 0}

    def dim(rgb, light_level, distance):
        d = int(distance) & 0xFFFF
        return (d & 255, d >> 8, state["kind"])

    def tagged(fn, kind):
        def call(*a, **k):
            state["kind"] = kind
            return fn(*a, **k)
        return call

    with mock.patch.object(nm, "diminish_color", dim), \
            mock.patch.object(nm, "render_vertical_bitmap_line", tagged(nm.render_vertical_bitmap_line, 1)), \
            mock.patch.object(nm, "draw_visplane", tagged(nm.draw_visplane, 2)):
        yield


def decode(px: np.ndarray):
    """Frame.px as the patched mappers left it -> (int16 distance [H, W], uint8 kind [H, W])."""
    kind = px[:, :, 2].copy()
    dist = (px[:, :, 0].astype(np.uint16) | (px[:, :, 1].astype(np.uint16) << 8)).view(np.int16).copy()
    dist[kind == 0] = FAR
    return dist, kind


def depth_of_lists(wad: bytes, sky_name: str, W: int, H: int, view: dict, lists: dict):
    """The planes of one list dict (the form np_mappers.draw_lists replays)."""
    with depth_mappers():
        return decode(nm.draw_lists(DepthWad(wad), sky_name, W, H, view, lists))


def written_mask(wad: bytes, sky_name: str, W: int, H: int, view: dict, lists: dict) -> np.ndarray:
    """Where the COLOUR path of np_mappers.draw_lists wrote a pixel (whatever its colour)."""
    Tracker.made.clear()
    with mock.patch.object(nm, "Frame", Tracker):
        nm.draw_lists(nm.Wad(wad), sky_name, W, H, view, lists)
    return Tracker.made.pop().writer >= 0


# ---- whole frames from dg_build_lists output: bitmap / flat ids back to the WAD's names ------------------------------------------

def _texture_names(np_wad):
    names = []
    for lump in ("TEXTURE1", "TEXTURE2"):
        try:
            t = np_wad.lump(lump)
        except KeyError:
            continue
        for i in range(struct.unpack_from("<I", t, 0)[0]):
            o = struct.unpack_from("<I", t, 4 + 4 * i)[0]
            names.append(t[o:o + 8].split(b"\0")[0].decode("ascii").upper())
    return names


class SceneNames:
    """Reverse maps of a dg scene's ids: bitmap id -> (w, h, rows) of the numpy decoders, flat id -> name, and the sprite ids."""

    def __init__(self, dg, scene, wad: bytes, nf):
        self.np_wad = DepthWad(wad)
        L = dg.lib()
        self.bitmaps, self.sprite_ids, self.flats = {}, set(), {}
        for name in _texture_names(self.np_wad):
            tid = L.dg_scene_texture_id(scene._h, name.encode())
            if tid >= 0 and tid not in self.bitmaps:
                self.bitmaps[tid] = self.np_wad.texture(name)
        sprites = nf.SpriteTable(wad)
        for i in range(sprites.first + 1, sprites.last_idx):
            lump = sprites.lumps[i][0]
            for (sprite, frame) in {(lump[:4], ord(lump[4]) - 65)} | ({(lump[:4], ord(lump[6]) - 65)} if len(lump) > 6 else set()):
                for rot in range(8):
                    bid = L.dg_scene_sprite_bitmap_id(scene._h, sprite.encode(), frame, rot)
                    if bid >= 0 and bid not in self.bitmaps:
                        w, h, _top, px = sprites.get_picture(sprite, frame, rot)
                        self.bitmaps[bid] = (w, h, px)
                        self.sprite_ids.add(bid)
        names = [n for (n, _o, _s) in self.np_wad.lumps]
        lo, hi = len(names) - 1 - names[::-1].index("F_START"), len(names) - 1 - names[::-1].index("F_END")
        for name in names[lo + 1:hi]:
            for ts in (0.0, 0.34, 0.67, 1.01):                       # every frame of an animated flat (flats.rs:103-111: timestamp * 3)
                fid = L.dg_scene_flat_id(scene._h, name.encode(), ts)
                if fid >= 0:
                    self.flats[fid] = nf.get_animated(name, ts)
        self.flat_cache = {}

    def flat(self, name):
        if name not in self.flat_cache:
            self.flat_cache[name] = self.np_wad.flat(name)
        return self.flat_cache[name]


def depth_of_frame_lists(names: SceneNames, sky_name: str, W: int, H: int, fl):
    """The planes of one dg_frame_lists (dg_build_lists output) -> (distance, kind, tracker); tracker.writer holds the index into
    fl.order of each pixel's last writer."""
    v = fl.view
    view = {"x": np.float32(v.x), "y": np.float32(v.y), "angle": np.float32(v.angle), "cos": np.float32(v.cos_a), "sin": np.float32(v.sin_a),
            "floor_height": np.float32(v.floor_height)}
    fr = Tracker(W, H)
    Tracker.made.clear()
    pal = names.np_wad.palette()
    sky = names.np_wad.texture(sky_name)
    with depth_mappers():
        for t in range(fl.n_order):
            fr.current = t
            cmd = fl.order[t]
            if cmd.kind == 0:
                r = fl.renders[cmd.index]
                rec = {"line": (r.line_start_x, r.line_start_y, r.line_end_x, r.line_end_y), "start_offset": r.start_offset, "start_x": r.start_x, "end_x": r.end_x,
                       "bottom_height": r.bottom_height, "top_height": r.top_height, "offset_x": r.offset_x, "offset_y": r.offset_y, "light_level": r.light_level}
                for i in range(r.first_column, r.first_column + r.n_columns):
                    c = fl.columns[i]
                    nm.render_vertical_bitmap_line(fr, names.bitmaps[r.bitmap], pal, rec, (c.x, c.clipped_top_y, c.clipped_bottom_y, c.bottom_y, c.top_y))
            else:
                p = fl.visplanes[cmd.index]
                tb = [(fl.plane_tb[2 * (p.first_entry + i)], fl.plane_tb[2 * (p.first_entry + i) + 1]) for i in range(p.right - p.left + 1)]
                name = names.flats[p.flat]
                d = {"flat": name, "height": p.height, "light_level": p.light_level, "left": p.left, "right": p.right, "tb": tb}
                if "SKY" in name:
                    nm.draw_sky(fr, sky, pal, view, d)
                else:
                    nm.draw_visplane(fr, names.flat(name), pal, view, d)
    dist, kind = decode(fr.px)
    return dist, kind, fr
