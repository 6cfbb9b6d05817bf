"""ctypes binding of the CPU test harness tests/emul/libdgemul.so (product host logic + kernel bodies on the CPU)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "emul", "libdgemul.so")
_lib = None


class DgView(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in "x y angle floor_height cos_a sin_a cos_na sin_na timestamp".split()] + \
               [("trig_valid", ctypes.c_int32)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "emul"), "-s"])
        L = ctypes.CDLL(_LIB)
        L.emul_load.restype = ctypes.c_void_p
        L.emul_load.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
        L.emul_free.argtypes = [ctypes.c_void_p]
        L.emul_last_error.restype = ctypes.c_char_p
        L.emul_render.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.emul_render_fe.argtypes = L.emul_render.argtypes
        L.emul_render_fe_slots.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.emul_draw_lists.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.emul_observe_lists.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
        L.emul_render_state.argtypes =[ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p]
        L.emul_fs_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(ctypes.c_uint64)]
        L.emul_frame_part_records.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_void_p, ctypes.c_int]
        L.emul_build_parts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView)]
        L.emul_fs_no_cl_rows.argtypes = [ctypes.c_int]
        L.emul_fs_no_cl_rows.restype = None
        L.emul_fs_kept_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.emul_sprite_frame.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint8]
        L.emul_set_wall_effects.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.emul_set_sector_light.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int16]
        L.emul_set_mobj_state.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_int]
        _lib = L
    return _lib


# emul_observe_lists (emul.cpp): stage-1 paths of dg_raster_tiles per (column, tile row), their overlay flags, why a span is not plain, pixel flags
PATHS = {"EMPTY": 0, "SOLE_WALL": 1, "SOLE_FLAT": 2, "WALK": 3, "BIG": 4, "PACKED": 5}
PATH_MASK, OV_WALK, OV_HIT, OV_UNDER = 7, 0x10, 0x20, 0x40
REASONS = {"npot": 1, "d0": 2, "first_out": 4, "last_out": 8, "gwz_out": 16, "wzvx_out": 32, "light7": 64}
PF_SHOWS, PF_BEFORE, PF_HOLE = 1, 2, 4


def fs_kept_counts(survivors, sky):
    """dg_fs_frame's survivor counting (fs_frame.h phases 2f / 2g) on the CPU for a made-up frame: lane l's slice of the candidate list
    holds survivors[l] kept candidates, sky[l] of them wanting a sky slot (FS_LANES = 256 lanes).  -> (fail, n_parts, n_sky)."""
    s = np.ascontiguousarray(survivors, dtype=np.uint32)
    k = np.ascontiguousarray(sky, dtype=np.uint32)
    assert s.shape == k.shape == (256,)
    out = np.zeros(3, dtype=np.uint32)
    if lib().emul_fs_kept_counts(s.ctypes.data, k.ctypes.data, out.ctypes.data):
        raise ValueError("more sky survivors than survivors in a lane")
    return int(out[0]), int(out[1]), int(out[2])


class EmulScene:
    def __init__(self, wad: bytes, map_name="e1m1"):
        self._h = lib().emul_load(wad, len(wad), map_name.encode())
        if not self._h:
            raise RuntimeError(lib().emul_last_error().decode())

    def set_sector_light(self, sector, light):
        lib().emul_set_sector_light(self._h, sector, light)

    def set_wall_effects(self, flags):
        """Scene::set_wall_effects (dg_scene_set_wall_effects): fs_frame then runs the seg walk's wall-effect variant."""
        if lib().emul_set_wall_effects(self._h, flags):
            raise RuntimeError(lib().emul_last_error().decode())

    def set_mobj_state(self, mobj, sprite, frame=0, full_bright=False):
        if lib().emul_set_mobj_state(self._h, mobj, sprite.encode() if sprite else None, frame, int(full_bright)):
            raise RuntimeError(lib().emul_last_error().decode())

    def render(self, W, H, rec, timestamp=0.0):
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        buf = np.empty(3 * W * H, dtype=np.uint8)
        st = (ctypes.c_uint64 * 4)()
        rc = lib().emul_render(self._h, W, H, ctypes.byref(v), buf.ctypes.data_as(ctypes.c_void_p), st)
        if rc:
            raise RuntimeError(f"emul rc {rc}: {lib().emul_last_error().decode()}")
        return buf.tobytes(), list(st)

    def draw_lists(self, W, H, frame_lists):
        """One dg_frame_lists (the ctypes structure of the package, as test_edge_kats.to_dg_lists makes it) through the binner and the
        kernel bodies: what dg_draw_lists takes.  The texture and flat ids are those of the same WAD loaded by the product."""
        buf = np.empty(3 * W * H, dtype=np.uint8)
        st = (ctypes.c_uint64 * 4)()
        rc = lib().emul_draw_lists(self._h, W, H, ctypes.byref(frame_lists), buf.ctypes.data_as(ctypes.c_void_p), st)
        if rc:
            raise RuntimeError(f"emul rc {rc}: {lib().emul_last_error().decode()}")
        return buf.tobytes(), list(st)

    def observe_lists(self, W, H, frame_lists):
        """What the product's own code decides for one dg_frame_lists, without drawing (emul.cpp emul_observe_lists) -> dict:
        `spans` (n, 8) uint32 rows = x, ctop, cbot, kind (0 wall, 1 flat, 2 sky), plain, immediate, reason, rec — from the DevRSpan word 0 of
        bin_frame + resolve_*_span, in the kernel's column-major order; reason (REASONS) is why a span is not plain; rec the span's draw call
        (n-th wall command / n-th non-sky visplane command of the order list);
        `chunks` (tile rows, W) uint8 = PATHS code | OV_* flags: the stage-1 path strip_body takes for the (column, 64-row tile);
        `owner` (H, W) int32 = row of `spans` of the last opaque span on the pixel, -1 for none;
        `pflags` (H, W) uint8: PF_SHOWS an overlay drawn after the owner shows, PF_BEFORE one was drawn before the owner, PF_HOLE one drawn
        after the owner has a transparent texel here."""
        cap = 1 << 16
        spans = np.zeros((cap, 8), dtype=np.uint32)
        chunks = np.zeros(((H + 63) // 64, W), dtype=np.uint8)
        owner = np.zeros((H, W), dtype=np.int32)
        pflags = np.zeros((H, W), dtype=np.uint8)
        n = lib().emul_observe_lists(self._h, W, H, ctypes.byref(frame_lists), spans.ctypes.data, cap, chunks.ctypes.data, owner.ctypes.data, pflags.ctypes.data)
        if n < 0:
            raise RuntimeError(f"emul_observe_lists rc {n}: {lib().emul_last_error().decode()}")
        return {"spans": spans[:n].copy(), "chunks": chunks, "owner": owner, "pflags": pflags}

    def sprite_frame(self, sprite, frame=0):
        sf = lib().emul_sprite_frame(self._h, sprite.encode(), frame)
        if sf < 0:
            raise RuntimeError(lib().emul_last_error().decode())
        return sf

    def render_state(self, W, H, rec, lights, mobjs, timestamp=0.0):
        """One view with a game-state snapshot: lights = [(sector, level)], mobjs = [(mobj, sprite_frame or -1, full_bright)]."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        la = np.array([[s, l] for s, l in lights], dtype=np.int32).reshape(-1, 2)
        ma = np.array([[m, sf, fb, 0] for m, sf, fb in mobjs], dtype=np.int32).reshape(-1, 4)
        buf = np.empty(3 * W * H, dtype=np.uint8)
        rc = lib().emul_render_state(self._h, W, H, ctypes.byref(v), la.ctypes.data, len(la), ma.ctypes.data, len(ma), buf.ctypes.data)
        if rc:
            raise RuntimeError(f"emul rc {rc}: {lib().emul_last_error().decode()}")
        return buf.tobytes()

    def fs_frame(self, W, H, rec, timestamp=0.0):
        """The device seg walk's bodies (fs_frame.h: dg_fs_segs / dg_fs_frame) on the CPU for one view, compared inside the
        harness with the host walker's parts mode record by record.  -> (rc, stats): rc 0 = identical records, 1 = the host walker
        refuses the frame and the device walk flagged it, 2 = the device walk gave the frame up because it exceeds a capacity (the host
        redoes it; stats[4] says which: 1 parts, 2 candidates, 4 sprites, 8 sky parts, 16 part bins, 32 sprite bins), 3 = it gave the frame
        up for no such reason; stats = [parts, sprites, sky slots, flags, capacities exceeded, candidates].  Raises on any mismatch."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        st = (ctypes.c_uint64 * 6)()
        rc = lib().emul_fs_frame(self._h, W, H, ctypes.byref(v), st)
        if rc < 0:
            raise RuntimeError(f"emul_fs_frame rc {rc}: {lib().emul_last_error().decode()}")
        return rc, list(st)

    def build_parts(self, W, H, rec, timestamp=0.0):
        """build_frame_parts (the host walker's parts mode) for one view -> (its return code, its error text)."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        rc = lib().emul_build_parts(self._h, W, H, ctypes.byref(v))
        return rc, lib().emul_last_error().decode()

    def frame_parts(self, W, H, rec, timestamp=0.0):
        """The host walker's FePart records of one view, whole (128 bytes each), with the scene's wall effects."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        out = np.zeros(128 * 4096, dtype=np.uint8)
        n = lib().emul_frame_part_records(self._h, W, H, ctypes.byref(v), out.ctypes.data, 4096)
        if n < 0:
            raise RuntimeError(f"emul_frame_part_records rc {n}: {lib().emul_last_error().decode()}")
        return out[:128 * n].tobytes()

    def render_fe(self, W, H, rec, timestamp=0.0):
        """Same frame through the device column walk's bodies (fe_core.h) on the CPU.  stats = [spans, parts, sprites, overflow
        flags, span-list-identical-to-host-path, sky gap entries]."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        buf = np.empty(3 * W * H, dtype=np.uint8)
        st = (ctypes.c_uint64 * 6)()
        rc = lib().emul_render_fe(self._h, W, H, ctypes.byref(v), buf.ctypes.data_as(ctypes.c_void_p), st)
        if rc:
            raise RuntimeError(f"emul rc {rc}: {lib().emul_last_error().decode()}")
        return buf.tobytes(), list(st)

    def fe_walk_counts(self, W, H, rec, slots=48, timestamp=0.0):
        """render_fe with `slots` column slots (DOOMGPU_FE_COLUMN_SLOTS) and the product's span list share (24 x W), plus counts taken
        next to the walk's bodies: where the frame's records put each of its loops.  -> (frame bytes, stats as render_fe's, counts);
        a frame that exceeds its span list share is flagged (stats[3] & 4) and not drawn (zeros).  counts: per column `nsp` (spans of the
        walk), `nrec`, `gaps` (sky gap entries), `sprite_spans`, `last_word` (sprite spans whose extent a wall record of the behind
        row's last word decides), `equal_keys`; per 64-column bin `parts`, `sprites`, `closed_at` (1-based list position of the part
        behind which no column of the bin is open; 0: it stayed open), `sky_behind` (sky parts listed behind that); and `n_parts`,
        `n_sprites`, `behind_words`, `sky_slots`, `flags`, `total`, `n_gaps`, `far_gaps` (gap entries whose scan leaves their word)."""
        v = DgView(float(rec[0]), float(rec[1]), float(rec[2]), float(rec[7]), float(rec[3]), float(rec[4]), float(rec[5]), float(rec[6]),
                   float(timestamp), 1)
        buf = np.zeros(3 * W * H, dtype=np.uint8)
        st = (ctypes.c_uint64 * 6)()
        w64 = (W + 63) // 64
        percol, perbin, misc = np.zeros((6, W), dtype=np.uint32), np.zeros((4, w64), dtype=np.uint32), np.zeros(8, dtype=np.uint64)
        rc = lib().emul_render_fe_slots(self._h, W, H, ctypes.byref(v), slots, buf.ctypes.data, st, percol.ctypes.data, perbin.ctypes.data, misc.ctypes.data)
        if rc:
            raise RuntimeError(f"emul rc {rc}: {lib().emul_last_error().decode()}")
        counts = dict(zip("nsp nrec gaps sprite_spans last_word equal_keys".split(), percol))
        counts.update(zip("parts sprites closed_at sky_behind".split(), perbin))
        counts.update(zip("n_parts n_sprites behind_words sky_slots flags total n_gaps far_gaps".split(), (int(m) for m in misc)))
        return buf.tobytes(), list(st), counts
