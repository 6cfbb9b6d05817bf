"""np_labels.py — the model of the object-label frame (include/doomgpu.h: dg_label_*).

Test infrastructure, in two independent halves.

  who owns a pixel   np_depth.depth_of_frame_lists replays a dg_frame_lists through np_mappers.py and records, per pixel, the index into
                     `order` of the draw command that wrote it last (overwrite order, transparency, clamps and the column rules are
                     np_mappers' own and share nothing with csrc/plane_core.h).  `labels_of_frame_lists` maps that index through
                     order -> render -> owner tag for the class and id of a column pixel; the class of flat and sky pixels comes from the
                     model's kind plane.  Boxes are plain numpy over the two planes.

  who owns a record  the tags frontend.cpp hands out are checked by leave-one-in runs of np_front_end.py (`lone_seg_records`,
                     `lone_thing_records`): seg k on a copy of the Map in which every other seg's linedef has no sides yields exactly the
                     records seg k makes (line, start_x, end_x, heights, texture: none of them depends on any other seg — only the
                     clipped columns do, and those are not compared); thing k alone in render_frame yields its one record.
"""
import copy
from unittest import mock

import numpy as np

import np_depth
import np_front_end as nf

NONE, WALL, MOBJ, FLAT, SKY = 0, 1, 2, 3, 4
BOX_DTYPE = np.dtype([("pixels", "<u4"), ("x0", "<i2"), ("y0", "<i2"), ("x1", "<i2"), ("y1", "<i2")])


def boxes_of(ids: np.ndarray, cls: np.ndarray, n_mobjs: int) -> np.ndarray:
    """Per map object: the number of pixels with class MOBJ and its id, and their inclusive bounding box (-1 four times when none)."""
    out = np.zeros(n_mobjs, dtype=BOX_DTYPE)
    for m in range(n_mobjs):
        ys, xs = np.nonzero((cls == MOBJ) & (ids == m))
        out[m] = (len(ys), xs.min(), ys.min(), xs.max(), ys.max()) if len(ys) else (0, -1, -1, -1, -1)
    return out


def labels_of_frame_lists(names, sky_name: str, W: int, H: int, fl, owners, n_mobjs: int):
    """-> (uint16 id [H, W], uint8 cls [H, W], boxes [n_mobjs], tracker, kind plane) of one dg_frame_lists with the owner tag of every
    render record."""
    _dist, kind, tr = np_depth.depth_of_frame_lists(names, sky_name, W, H, fl)
    ids = np.zeros((H, W), dtype=np.uint16)
    cls = np.zeros((H, W), dtype=np.uint8)
    cls[kind == 2] = FLAT
    cls[kind == 3] = SKY
    for t in range(fl.n_order):
        cmd = fl.order[t]
        if cmd.kind != 0:
            continue
        mine = tr.writer == t
        tag = int(owners[cmd.index])
        cls[mine] = tag >> 16
        ids[mine] = tag & 0xFFFF
    assert ((cls == NONE) == (tr.writer < 0)).all() and ((kind == 1) == ((cls == WALL) | (cls == MOBJ))).all()
    return ids, cls, boxes_of(ids, cls, n_mobjs), tr, kind


# ---- leave-one-in runs of np_front_end --------------------------------------------------------------------------------------------------

_NO_SIDES = {"flags": 0, "front": None, "back": None}


def _record(c, texture):
    return tuple(np.float32(t) for t in c["line"]) + (int(c["start_x"]), int(c["end_x"]), np.float32(c["bottom_height"]), np.float32(c["top_height"]), texture)


def lone_seg_records(m: nf.Map, k: int, W: int, H: int, view):
    """The drawable records of seg k alone (textured, not occlusion-only: what BitmapRender::new is given and a draw can replay)."""
    lone = copy.copy(m)
    lone.segs = [s if i == k else dict(s, linedef=_NO_SIDES) for i, s in enumerate(m.segs)]
    calls = nf.per_seg_calls(lone, W, H, view)
    return [_record(c, c["texture"]) for c in calls if (c["flags"] & nf.HAS_TEXTURE) and not (c["flags"] & nf.ONLY_OCCLUSIONS)]


class _Recorder:
    """Stands in for np_mappers in np_front_end.render_frame: draws nothing, keeps every column draw call's record and bitmap."""

    class Frame:
        def __init__(self, W, H):
            self.px = None

    def __init__(self):
        self.calls = []

    def render_vertical_bitmap_line(self, fr, bitmap, pal, rec, col):
        self.calls.append((rec, bitmap))

    def draw_sky(self, *a):
        pass

    def draw_visplane(self, *a):
        pass


def lone_thing_records(m: nf.Map, thing, sprites, np_wad, W: int, H: int, view, walls):
    """The records of one thing alone in the frame: [(record, (sprite, frame, rotation))].  `walls`: the (calls, columns) of the view,
    computed once by the caller — render_frame would walk the map again for every thing."""
    asked = []
    get = sprites.get_picture

    def get_picture(sprite, frame, rotation):
        pic = get(sprite, frame, rotation)
        asked.append((pic, (sprite, frame, rotation)))
        return pic

    rec = _Recorder()
    with mock.patch.object(nf, "per_seg_calls", lambda *a: walls[0]), mock.patch.object(nf, "column_loops", lambda *a: (walls[1], [])), \
            mock.patch.object(sprites, "get_picture", get_picture):
        nf.render_frame(m, [thing], sprites, np_wad, rec, W, H, view)
    out = []
    for (r, bitmap) in rec.calls:
        which = [key for (pic, key) in asked if pic[0] == bitmap[0] and pic[1] == bitmap[1] and pic[3] is bitmap[2]]
        if which and (_record(r, which[0]) not in out):
            out.append(_record(r, which[0]))
    return out


def bitmap_id(dg, scene, what) -> int:
    """The scene's bitmap id of what a lone-run record draws: a texture name, or a (sprite, frame, rotation)."""
    if isinstance(what, str):
        return dg.lib().dg_scene_texture_id(scene._h, what.encode())
    return dg.lib().dg_scene_sprite_bitmap_id(scene._h, what[0].encode(), what[1], what[2])


def render_record(r):
    """A dg_bitmap_render in the form the lone runs' records take once their last entry went through bitmap_id."""
    return tuple(np.float32(t) for t in (r.line_start_x, r.line_start_y, r.line_end_x, r.line_end_y)) + \
        (int(r.start_x), int(r.end_x), np.float32(r.bottom_height), np.float32(r.top_height), int(r.bitmap))
