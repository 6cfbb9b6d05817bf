"""doom-rust-renderer_amd — MI355X-native column/span rasteriser behind the reference's Pixels/Renderer draw API.

This Python module is only the test/bench harness binding (ctypes) of the C-ABI in ``include/doomgpu.h``;
the product is ``libdoomgpu.so`` (hand-written HIP kernels + C++ host list generation, ``csrc/``).
Import with ``importlib.import_module("doom-rust-renderer_amd")`` (the directory name carries a hyphen).

There is no CPU fallback anywhere in this package: without the built library every call raises, and without
a gfx950 device ``Context`` raises ``DoomGpuError`` (DG_ERR_NO_DEVICE).  The oracle under ``oracle/`` is never
imported from here.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DOOMGPU_LIB") or os.path.join(_HERE, "libdoomgpu.so")   # override only for kernel-variant experiments
INCLUDE = os.path.join(os.path.dirname(_HERE), "include", "doomgpu.h")

DG_OK, DG_ERR_INVALID, DG_ERR_NO_DEVICE, DG_ERR_HIP, DG_ERR_WAD, DG_ERR_RENDER, DG_ERR_CAPACITY, DG_ERR_STATE = 0, -1, -2, -3, -4, -5, -6, -7
DG_FE_AUTO, DG_FE_HOST, DG_FE_DEVICE, DG_FE_DEVICE_SEGS = 0, 1, 2, 3
DG_FE_MAP = 4   # dg_timing.front_end of a 2-D map submission
DG_FE_DEPTH = 5  # dg_timing.front_end of a depth submission
DG_KIND_NONE, DG_KIND_COLUMN, DG_KIND_FLAT, DG_KIND_SKY = 0, 1, 2, 3   # the kind plane of a depth frame
DG_FE_LABELS = 6  # dg_timing.front_end of a label submission
DG_LABEL_NONE, DG_LABEL_WALL, DG_LABEL_MOBJ, DG_LABEL_FLAT, DG_LABEL_SKY = 0, 1, 2, 3, 4   # the class plane of a label frame / the class of an owner tag
DG_FE_BUNDLE = 7  # dg_timing.front_end of a bundle submission
DG_BUNDLE_COLOUR, DG_BUNDLE_DEPTH, DG_BUNDLE_LABELS = 1, 2, 4   # the parts of a bundle submission (`what`)
# dg_label_box as a numpy record: boxes come back as an (n, map objects) array of these
LABEL_BOX_DTYPE = np.dtype([("pixels", "<u4"), ("x0", "<i2"), ("y0", "<i2"), ("x1", "<i2"), ("y1", "<i2")])
DG_FE_MAP_EXPLORED = 8  # dg_timing.front_end of an explored-map submission
DG_FE_MAP_EGO = 9  # dg_timing.front_end of a player-centred map submission
DG_FE_MAP_FLOOR = 10  # dg_timing.front_end of a floor-textured player-centred map submission
DG_EGO_ROTATE, DG_EGO_ARROW = 1, 2   # dg_ego_map.flags
DG_MARK_BOX, DG_MARK_HEADING = 1, 2   # dg_map_marker.flags
DG_WALL_ANIMATE, DG_WALL_SCROLL = 1, 2   # dg_scene_set_wall_effects flags
DG_LIGHT_THINKERS = 1                    # dg_scene_set_light_effects flag
DG_MOBJ_THINKERS = 1                     # dg_scene_set_mobj_thinkers flag
DG_MOBJ_KILL, DG_MOBJ_EXPLODE, DG_MOBJ_RESPAWN = 1, 2, 3   # dg_scene_mobj_event
DG_REDUCE_RGB24, DG_REDUCE_GRAY8 = 0, 1  # dg_reduce_desc.format
DG_PLANE_POINT, DG_PLANE_NEAREST = 0, 1  # dg_plane_reduce_desc.rule
DG_OBS_RGB, DG_OBS_GRAY, DG_OBS_DISTANCE = 0, 1, 2  # dg_obs_desc.source
DG_OBS_U8, DG_OBS_F16, DG_OBS_BF16, DG_OBS_F32 = 0, 1, 2, 3  # dg_obs_desc.dtype
DG_KEY_LEFT, DG_KEY_RIGHT, DG_KEY_UP, DG_KEY_DOWN, DG_KEY_ALT, DG_KEY_SHIFT = 1, 2, 4, 8, 16, 32   # dg_walk_desc.keys


class DoomGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"doomgpu error {code}: {msg}")
        self.code = code


class DgView(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in "x y angle floor_height cos_a sin_a cos_na sin_na timestamp".split()] + \
               [("trig_valid", ctypes.c_int32)]


class DgSectorLight(ctypes.Structure):
    _fields_ = [("sector", ctypes.c_int32), ("light_level", ctypes.c_int32)]


class DgMobjState(ctypes.Structure):
    _fields_ = [("mobj", ctypes.c_int32), ("sprite_frame", ctypes.c_int32), ("full_bright", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DgStateRec(ctypes.Structure):
    _fields_ = [("sprite", ctypes.c_char * 4), ("frame", ctypes.c_uint8), ("full_bright", ctypes.c_uint8), ("tics", ctypes.c_int16),
                ("next_state", ctypes.c_int32)]


class DgMobjInfoRec(ctypes.Structure):
    _fields_ = [("doomednum", ctypes.c_int32), ("spawn_state", ctypes.c_int32), ("death_state", ctypes.c_int32), ("xdeath_state", ctypes.c_int32)]


class DgViewState(ctypes.Structure):
    _fields_ = [("lights", ctypes.POINTER(DgSectorLight)), ("n_lights", ctypes.c_uint32),
                ("mobjs", ctypes.POINTER(DgMobjState)), ("n_mobjs", ctypes.c_uint32)]


class DgMobjPose(ctypes.Structure):
    _fields_ = [("mobj", ctypes.c_int32), ("x", ctypes.c_float), ("y", ctypes.c_float), ("angle", ctypes.c_float)]


class DgViewPoses(ctypes.Structure):
    _fields_ = [("poses", ctypes.POINTER(DgMobjPose)), ("n", ctypes.c_uint32)]


class DgMobjPlaced(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("angle", ctypes.c_float), ("sector", ctypes.c_int32)]


class DgSectorHeights(ctypes.Structure):
    _fields_ = [("sector", ctypes.c_int32), ("floor_height", ctypes.c_int32), ("ceiling_height", ctypes.c_int32)]


class DgViewSectors(ctypes.Structure):
    _fields_ = [("heights", ctypes.POINTER(DgSectorHeights)), ("n", ctypes.c_uint32)]


TEX_NONE = -1   # DG_TEX_NONE: "-"


class DgSideSurface(ctypes.Structure):
    _fields_ = [("sidedef", ctypes.c_int32), ("tex_mid", ctypes.c_int32), ("tex_low", ctypes.c_int32), ("tex_up", ctypes.c_int32),
                ("x_offset", ctypes.c_int32), ("y_offset", ctypes.c_int32)]


class DgSectorFlats(ctypes.Structure):
    _fields_ = [("sector", ctypes.c_int32), ("floor_flat", ctypes.c_int32), ("ceil_flat", ctypes.c_int32)]


class DgViewSurfaces(ctypes.Structure):
    _fields_ = [("sides", ctypes.POINTER(DgSideSurface)), ("n_sides", ctypes.c_uint32), ("flats", ctypes.POINTER(DgSectorFlats)), ("n_flats", ctypes.c_uint32)]


# a row of dg_mobj_placed as numpy sees it (dg_scene_mobj_poses, dg_slot_mobj_poses)
MOBJ_PLACED_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("sector", "<i4")])


class DgWalkDesc(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("angle", ctypes.c_float), ("from_player_start", ctypes.c_int32),
                ("turbo", ctypes.c_int32), ("keys", ctypes.POINTER(ctypes.c_uint8)), ("n_tics", ctypes.c_uint32)]


class DgReduceDesc(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_uint32), ("fy", ctypes.c_uint32), ("format", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DgPlaneReduceDesc(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_uint32), ("fy", ctypes.c_uint32), ("rule", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DgObsDesc(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_uint32), ("fy", ctypes.c_uint32), ("source", ctypes.c_uint32), ("rule", ctypes.c_uint32), ("dtype", ctypes.c_uint32),
                ("lo", ctypes.c_int32), ("hi", ctypes.c_int32), ("scale", ctypes.c_float), ("bias", ctypes.c_float), ("reserved", ctypes.c_uint32)]


DG_PIC_OFFSETS = 1                       # dg_screen_picture.flags: the origin moves by the picture's offsets times the scale
DG_PIC_MIRROR = 2                        # ... texel column w-1-tx
# dg_screen_picture, one item of a frame's screen pictures
SCREEN_PICTURE_DTYPE = np.dtype([("picture", "<i4"), ("x", "<i4"), ("y", "<i4"), ("scale_x", "<u2"), ("scale_y", "<u2"), ("light_level", "<i2"), ("flags", "<u2")])


class DgBundleOffsets(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in "colour distance kind id cls total".split()]


class DgConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in "device width height max_batch slots host_threads front_end".split()]


class DgTiming(ctypes.Structure):
    _fields_ = [("setup_ms", ctypes.c_float), ("raster_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("host_ms", ctypes.c_float),
                ("n_spans", ctypes.c_uint64), ("n_frames", ctypes.c_uint64), ("covered_pixels", ctypes.c_uint64),
                ("n_walls", ctypes.c_uint64), ("n_planes", ctypes.c_uint64), ("list_bytes", ctypes.c_uint64),
                ("front_end", ctypes.c_int32)]


class DgMapLine(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in "x0 y0 x1 y1".split()] + [("rgb", ctypes.c_uint32)]


class DgEgoMap(ctypes.Structure):
    _fields_ = [("scale", ctypes.c_float), ("flags", ctypes.c_uint32)]


class DgMapMarker(ctypes.Structure):
    _fields_ = [("radius", ctypes.c_int32), ("rgb", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class DgBitmapColumn(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int16) for n in "x clipped_top_y clipped_bottom_y bottom_y top_y".split()]


class DgBitmapRender(ctypes.Structure):
    _fields_ = [("bitmap", ctypes.c_int32), ("light_level", ctypes.c_int16), ("offset_x", ctypes.c_int16),
                ("offset_y", ctypes.c_int16), ("reserved", ctypes.c_int16),
                ("line_start_x", ctypes.c_float), ("line_start_y", ctypes.c_float), ("line_end_x", ctypes.c_float),
                ("line_end_y", ctypes.c_float), ("start_offset", ctypes.c_float), ("start_x", ctypes.c_int32),
                ("end_x", ctypes.c_int32), ("bottom_height", ctypes.c_float), ("top_height", ctypes.c_float),
                ("first_column", ctypes.c_uint32), ("n_columns", ctypes.c_uint32)]


class DgVisplane(ctypes.Structure):
    _fields_ = [("flat", ctypes.c_int32), ("height", ctypes.c_int16), ("light_level", ctypes.c_int16),
                ("left", ctypes.c_int16), ("right", ctypes.c_int16), ("first_entry", ctypes.c_uint32)]


class DgDrawCmd(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class DgFrameLists(ctypes.Structure):
    _fields_ = [("view", DgView),
                ("renders", ctypes.POINTER(DgBitmapRender)), ("n_renders", ctypes.c_uint32),
                ("columns", ctypes.POINTER(DgBitmapColumn)), ("n_columns", ctypes.c_uint32),
                ("visplanes", ctypes.POINTER(DgVisplane)), ("n_visplanes", ctypes.c_uint32),
                ("plane_tb", ctypes.POINTER(ctypes.c_int16)), ("n_plane_tb", ctypes.c_uint32),
                ("order", ctypes.POINTER(DgDrawCmd)), ("n_order", ctypes.c_uint32)]


def build(force: bool = False) -> str:
    """Compile libdoomgpu.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [INCLUDE]
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", csrc, "-s"])
    return LIB_PATH


_lib = None

# every symbol include/doomgpu.h declares: (restype, argtypes)
_P = ctypes.c_void_p
_SIGNATURES = {
    "dg_scene_load_wad": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(_P)]),
    "dg_scene_free": (None, [_P]),
    "dg_scene_player_start": (ctypes.c_int, [_P] + [ctypes.POINTER(ctypes.c_float)] * 3),
    "dg_scene_floor_height_at": (ctypes.c_int, [_P, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]),
    "dg_scene_sector_count": (ctypes.c_int, [_P]),
    "dg_scene_set_sector_light": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int16]),
    "dg_scene_mobj_count": (ctypes.c_int, [_P]),
    "dg_scene_set_mobj_state": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_int]),
    "dg_create": (ctypes.c_int, [ctypes.POINTER(DgConfig), ctypes.POINTER(_P)]),
    "dg_destroy": (None, [_P]),
    "dg_ctx_host_threads": (ctypes.c_int, [_P]),
    "dg_upload_scene": (ctypes.c_int, [_P, _P]),
    "dg_render_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, _P]),
    "dg_submit_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int]),
    "dg_submit_views_state": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int]),
    "dg_render_views_state": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int, _P]),
    "dg_scene_sprite_frame": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint8]),
    "dg_wait": (ctypes.c_int, [_P, ctypes.c_int]),
    "dg_slot_framebuffer": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    "dg_readback": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "dg_readback_async": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "dg_ctx_fallbacks": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "dg_ctx_redone_frames": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "dg_frame_checksums": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "dg_reduced_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgReduceDesc), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_size_t)]),
    "dg_reduce_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgReduceDesc), _P]),
    "dg_readback_reduced": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgReduceDesc), _P]),
    "dg_readback_reduced_async": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgReduceDesc), _P]),
    "dg_reduce_device": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgReduceDesc), _P]),
    "dg_ctx_reduce_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "dg_alloc_host": (_P, [ctypes.c_size_t]),
    "dg_free_host": (None, [_P]),
    "dg_prepare_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int]),
    "dg_replay_slot": (ctypes.c_int, [_P, ctypes.c_int]),
    "dg_scene_texture_id": (ctypes.c_int, [_P, ctypes.c_char_p]),
    "dg_scene_flat_id": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_float]),
    "dg_scene_set_wall_effects": (ctypes.c_int, [_P, ctypes.c_uint32]),
    "dg_scene_wall_texture_id": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_float]),
    "dg_scene_set_light_effects": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint64]),
    "dg_scene_sector_lights_at": (ctypes.c_int, [_P, ctypes.c_float, ctypes.POINTER(ctypes.c_int16), ctypes.c_int]),
    "dg_scene_set_mobj_thinkers": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(DgStateRec), ctypes.c_int, ctypes.POINTER(DgMobjInfoRec), ctypes.c_int]),
    "dg_scene_mobj_event": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_float]),
    "dg_scene_mobj_states_at": (ctypes.c_int, [_P, ctypes.c_float, ctypes.POINTER(DgMobjState), ctypes.c_int]),
    "dg_scene_sprite_bitmap_id": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_uint8]),
    "dg_scene_bitmap_size": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dg_draw_lists": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.c_int, _P]),
    "dg_build_lists": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgFrameLists)]),
    "dg_map_lines": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgMapLine), ctypes.c_int]),
    "dg_submit_map_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int]),
    "dg_render_map_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, _P]),
    "dg_submit_depth_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int]),
    "dg_render_depth_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int, _P, _P]),
    "dg_depth_lists": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.c_int, _P, _P]),
    "dg_readback_depth": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "dg_depth_lists_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.c_int, _P, _P]),
    "dg_build_lists_poses": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgFrameLists), ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]),
    "dg_scene_sectors_at": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, _P]),
    "dg_scene_mobj_poses": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "dg_submit_views_poses": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.c_int]),
    "dg_render_views_poses": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.c_int, _P]),
    "dg_submit_bundle_views_poses": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.c_int, ctypes.c_uint32]),
    "dg_slot_mobj_poses": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "dg_slot_mobj_pose_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "dg_build_lists_sectors": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.POINTER(DgFrameLists), ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]),
    "dg_scene_sector_heights": (ctypes.c_int, [_P, _P, _P, ctypes.c_int]),
    "dg_submit_views_sectors": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.c_int]),
    "dg_render_views_sectors": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.c_int, _P]),
    "dg_submit_bundle_views_sectors": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.c_int, ctypes.c_uint32]),
    "dg_slot_sector_heights": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "dg_slot_sector_height_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "dg_scene_use_texture": (ctypes.c_int, [_P, ctypes.c_char_p]),
    "dg_scene_use_flat": (ctypes.c_int, [_P, ctypes.c_char_p]),
    "dg_scene_sidedef_count": (ctypes.c_int, [_P]),
    "dg_scene_sidedef_surfaces": (ctypes.c_int, [_P, ctypes.POINTER(DgSideSurface), ctypes.c_int]),
    "dg_scene_sector_flats": (ctypes.c_int, [_P, ctypes.POINTER(DgSectorFlats), ctypes.c_int]),
    "dg_build_lists_surfaces": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.POINTER(DgViewSurfaces), ctypes.POINTER(DgFrameLists), ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]),
    "dg_submit_views_surfaces": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.POINTER(DgViewSurfaces), ctypes.c_int]),
    "dg_render_views_surfaces": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.POINTER(DgViewSurfaces), ctypes.c_int, _P]),
    "dg_submit_bundle_views_surfaces": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.POINTER(DgViewSurfaces), ctypes.c_int, ctypes.c_uint32]),
    "dg_slot_sector_flats": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "dg_slot_surface_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "dg_build_lists_owners": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgFrameLists), ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]),
    "dg_submit_label_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int]),
    "dg_render_label_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int, _P, _P, _P]),
    "dg_label_lists": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.POINTER(_P), ctypes.c_int, _P, _P, _P]),
    "dg_readback_labels": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "dg_slot_label_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "dg_label_lists_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.POINTER(_P), ctypes.c_int, _P, _P, _P]),
    "dg_bundle_layout": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(DgBundleOffsets)]),
    "dg_bundle_capacity": (ctypes.c_int, [_P, ctypes.c_uint32]),
    "dg_submit_bundle_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgViewState), ctypes.c_int, ctypes.c_uint32]),
    "dg_bundle_lists": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.POINTER(_P), ctypes.c_int, ctypes.c_uint32]),
    "dg_bundle_lists_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgFrameLists), ctypes.POINTER(_P), ctypes.c_int, _P, _P, _P, _P, _P]),
    "dg_slot_bundle_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "dg_plane_reduced_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgPlaneReduceDesc), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dg_reduce_planes_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgPlaneReduceDesc)] + [_P] * 8),
    "dg_reduce_planes_device": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgPlaneReduceDesc)] + [_P] * 8),
    "dg_ctx_plane_reduce_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "dg_observed_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgObsDesc)] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "dg_observe_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgObsDesc), _P, ctypes.POINTER(ctypes.c_int64)]),
    "dg_observe_device": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgObsDesc), _P, ctypes.POINTER(ctypes.c_int64)]),
    "dg_ctx_observe_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "dg_scene_use_picture": (ctypes.c_int, [_P, ctypes.c_char_p]),
    "dg_scene_picture_count": (ctypes.c_int, [_P]),
    "dg_scene_picture_info": (ctypes.c_int, [_P, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int32)] * 4),
    "dg_overlay_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "dg_overlay_device": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "dg_slot_overlay": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "dg_ctx_overlay_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "dg_readback_planes_reduced": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgPlaneReduceDesc)] + [_P] * 5),
    "dg_readback_planes_reduced_async": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgPlaneReduceDesc)] + [_P] * 5),
    "dg_seen_words": (ctypes.c_int, [_P]),
    "dg_seen_lines_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "dg_seen_accumulate_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_P] * 6),
    "dg_explored_map_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), _P, _P]),
    "dg_seen_lines_device": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "dg_slot_seen_lines": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_P] * 5),
    "dg_ctx_seen_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "dg_submit_explored_map_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int, _P]),
    "dg_render_explored_map_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, _P, _P]),
    "dg_ego_map_lines": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), ctypes.POINTER(DgMapLine), ctypes.c_int]),
    "dg_ego_map_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), _P, _P]),
    "dg_submit_ego_map_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P]),
    "dg_render_ego_map_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, _P]),
    "dg_floor_map_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                         ctypes.POINTER(DgViewSurfaces), _P]),
    "dg_submit_floor_map_views": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                 ctypes.POINTER(DgViewSurfaces)]),
    "dg_render_floor_map_views": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                 ctypes.POINTER(DgViewSurfaces), _P]),
    "dg_scene_set_map_markers": (ctypes.c_int, [_P, ctypes.POINTER(DgMapMarker), ctypes.c_int]),
    "dg_map_thing_lines": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), ctypes.POINTER(DgViewState),
                                          ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgMapLine), ctypes.c_int]),
    "dg_ego_map_things_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                              ctypes.POINTER(DgViewPoses), _P]),
    "dg_floor_map_things_host": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DgView), ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                ctypes.POINTER(DgViewSurfaces), ctypes.POINTER(DgViewPoses), _P]),
    "dg_submit_ego_map_views_things": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                      ctypes.POINTER(DgViewPoses)]),
    "dg_render_ego_map_views_things": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                      ctypes.POINTER(DgViewPoses), _P]),
    "dg_submit_floor_map_views_things": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                        ctypes.POINTER(DgViewSurfaces), ctypes.POINTER(DgViewPoses)]),
    "dg_render_floor_map_views_things": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.c_int, ctypes.POINTER(DgEgoMap), _P, ctypes.POINTER(DgViewState),
                                                        ctypes.POINTER(DgViewSurfaces), ctypes.POINTER(DgViewPoses), _P]),
    "dg_sight_host": (ctypes.c_int, [_P, ctypes.POINTER(DgViewSectors), ctypes.c_int, _P, ctypes.c_int, _P]),
    "dg_sight_device": (ctypes.c_int, [_P, ctypes.POINTER(DgViewSectors), ctypes.c_int, _P, ctypes.c_int, _P]),
    "dg_sight_words": (ctypes.c_int, [_P]),
    "dg_sight_mobjs_host": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.c_int, ctypes.c_float, _P, _P]),
    "dg_sight_mobjs_device": (ctypes.c_int, [_P, ctypes.POINTER(DgView), ctypes.POINTER(DgViewPoses), ctypes.POINTER(DgViewSectors), ctypes.c_int, ctypes.c_float, _P, _P]),
    "dg_ctx_sight_kernel_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "dg_scene_bsp_depth": (ctypes.c_int, [_P]),
    "dg_walk_create": (ctypes.c_int, [_P, ctypes.POINTER(DgWalkDesc), ctypes.POINTER(_P)]),
    "dg_walk_free": (None, [_P]),
    "dg_walk_tics": (ctypes.c_int, [_P]),
    "dg_walk_probe_count": (ctypes.c_int, [_P]),
    "dg_walk_floors": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
    "dg_walk_views": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(DgView)]),
    "dg_ctx_locate_walks": (ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.c_int]),
    "dg_last_error": (ctypes.c_char_p, []),
    "dg_version": (ctypes.c_char_p, []),
    "dg_slot_timing": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(DgTiming)]),
}


def lib():
    """Load libdoomgpu.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DoomGpuError(DG_ERR_NO_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() — there is no fallback path")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int):
    if rc < 0:
        raise DoomGpuError(rc, lib().dg_last_error().decode(errors="replace"))
    return rc


def _reduce_desc(desc) -> DgReduceDesc:
    """A DgReduceDesc as it is, or one from (fx, fy) / (fx, fy, format)."""
    return desc if isinstance(desc, DgReduceDesc) else DgReduceDesc(int(desc[0]), int(desc[1]), int(desc[2]) if len(desc) > 2 else DG_REDUCE_RGB24, 0)


def reduced_size(width: int, height: int, desc):
    """dg_reduced_size: (oW, oH, bytes per reduced frame) of a width x height frame under desc (a DgReduceDesc, or (fx, fy[, format]))."""
    w, h, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _check(lib().dg_reduced_size(width, height, ctypes.byref(_reduce_desc(desc)), ctypes.byref(w), ctypes.byref(h), ctypes.byref(b)))
    return w.value, h.value, b.value


def _reduced_array(count: int, width: int, height: int, d: DgReduceDesc) -> np.ndarray:
    ow, oh, _ = reduced_size(width, height, d)
    return np.empty((count, oh, ow) if d.format == DG_REDUCE_GRAY8 else (count, oh, ow, 3), dtype=np.uint8)


def reduce_host(frames, desc) -> np.ndarray:
    """dg_reduce_host: the box downscale on the CPU of frames (n, H, W, 3) uint8; returns (n, oH, oW, 3) or, as gray, (n, oH, oW)."""
    src = np.ascontiguousarray(frames, dtype=np.uint8)
    if src.ndim != 4 or src.shape[3] != 3:
        raise ValueError("frames must be (n, H, W, 3) uint8")
    d = _reduce_desc(desc)
    n, h, w, _ = src.shape
    out = _reduced_array(n, w, h, d)
    _check(lib().dg_reduce_host(src.ctypes.data_as(_P), w, h, n, ctypes.byref(d), out.ctypes.data_as(_P)))
    return out


PLANE_NAMES = ("distance", "kind", "id", "cls")
PLANE_DTYPES = {"distance": np.int16, "kind": np.uint8, "id": np.uint16, "cls": np.uint8}


def _plane_reduce_desc(desc) -> DgPlaneReduceDesc:
    """A DgPlaneReduceDesc as it is, or one from (fx, fy) / (fx, fy, rule)."""
    return desc if isinstance(desc, DgPlaneReduceDesc) else DgPlaneReduceDesc(int(desc[0]), int(desc[1]), int(desc[2]) if len(desc) > 2 else DG_PLANE_POINT, 0)


def plane_reduced_size(width: int, height: int, desc):
    """dg_plane_reduced_size: (oW, oH) of a width x height plane under desc (a DgPlaneReduceDesc, or (fx, fy[, rule]))."""
    w, h = ctypes.c_int(), ctypes.c_int()
    _check(lib().dg_plane_reduced_size(width, height, ctypes.byref(_plane_reduce_desc(desc)), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


# dg_obs_desc.dtype -> what observe_host returns (BF16: the bit patterns), and the name a tensor's dtype ends in (observe_into)
OBS_NP_DTYPES = {DG_OBS_U8: np.uint8, DG_OBS_F16: np.float16, DG_OBS_BF16: np.uint16, DG_OBS_F32: np.float32}
OBS_DTYPE_NAMES = {DG_OBS_U8: "uint8", DG_OBS_F16: "float16", DG_OBS_BF16: "bfloat16", DG_OBS_F32: "float32"}


def observed_size(width: int, height: int, desc: DgObsDesc):
    """dg_observed_size: (channels, oH, oW, element bytes) of the observation of a width x height source under desc."""
    c, h, w, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(lib().dg_observed_size(width, height, ctypes.byref(desc), ctypes.byref(c), ctypes.byref(h), ctypes.byref(w), ctypes.byref(b)))
    return c.value, h.value, w.value, b.value


def observe_host(src, desc: DgObsDesc) -> np.ndarray:
    """dg_observe_host: frames (n, H, W, 3) uint8 (DG_OBS_RGB, DG_OBS_GRAY) or distance planes (n, H, W) int16 (DG_OBS_DISTANCE) observed
    on the CPU; returns a contiguous (n, C, oH, oW) array of uint8, float16 or float32, and for DG_OBS_BF16 uint16 bit patterns."""
    colour = desc.source != DG_OBS_DISTANCE
    src = np.ascontiguousarray(src, dtype=np.uint8 if colour else np.int16)
    if src.ndim != (4 if colour else 3) or (colour and src.shape[3] != 3):
        raise ValueError("src must be (n, H, W, 3) uint8 frames, or (n, H, W) int16 distance planes for DG_OBS_DISTANCE")
    n, h, w = src.shape[:3]
    c, oh, ow, _ = observed_size(w, h, desc)
    out = np.empty((n, c, oh, ow), dtype=OBS_NP_DTYPES[desc.dtype])
    strides = (ctypes.c_int64 * 4)(c * oh * ow, oh * ow, ow, 1)
    _check(lib().dg_observe_host(src.ctypes.data_as(_P), w, h, n, ctypes.byref(desc), out.ctypes.data_as(_P), strides))
    return out


def screen_pictures(items_per_frame):
    """items[] and first[n + 1] of a batch's screen pictures from a list, one entry per frame, of lists of tuples
    (picture, x, y[, scale_x[, scale_y[, light_level[, flags]]]]) — scales default to 1, the light to 255, the flags to 0.
    Returns (items, first): a SCREEN_PICTURE_DTYPE array and a uint32 array."""
    defaults = (1, 1, 255, 0)
    rows, first = [], [0]
    for frame in items_per_frame:
        for it in frame:
            it = tuple(it)
            if not 3 <= len(it) <= 7:
                raise ValueError("a screen picture is (picture, x, y[, scale_x[, scale_y[, light_level[, flags]]]])")
            rows.append(it + defaults[len(it) - 3:])
        first.append(len(rows))
    items = np.array(rows, dtype=SCREEN_PICTURE_DTYPE) if rows else np.zeros(0, dtype=SCREEN_PICTURE_DTYPE)
    return items, np.array(first, dtype=np.uint32)


def overlay_host(scene, frames, items_per_frame):
    """dg_overlay_host: the screen pictures items_per_frame (screen_pictures) drawn in place on frames, an (n, H, W, 3) uint8
    C-contiguous array with one list per frame; returns frames."""
    if not (isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3 and frames.flags.c_contiguous and frames.flags.writeable):
        raise ValueError("frames must be a writeable C-contiguous (n, H, W, 3) uint8 array")
    n, h, w, _ = frames.shape
    if len(items_per_frame) != n:
        raise ValueError("one list of screen pictures per frame")
    items, first = screen_pictures(items_per_frame)
    _check(lib().dg_overlay_host(scene._h, frames.ctypes.data_as(_P), w, h, n, items.ctypes.data_as(_P), first.ctypes.data_as(_P)))
    return frames


def reduce_planes_host(desc, distance=None, kind=None, id=None, cls=None) -> dict:
    """dg_reduce_planes_host: the planes that are given, each (n, H, W) — distance int16, kind uint8, id uint16, cls uint8 — reduced on
    the CPU under desc (a DgPlaneReduceDesc, or (fx, fy[, rule])); returns {name: (n, oH, oW) array} for the planes given."""
    d = _plane_reduce_desc(desc)
    src = {k: np.ascontiguousarray(v, dtype=PLANE_DTYPES[k]) for k, v in zip(PLANE_NAMES, (distance, kind, id, cls)) if v is not None}
    if not src:
        raise ValueError("no plane given")
    n, h, w = next(iter(src.values())).shape
    if any(a.shape != (n, h, w) for a in src.values()):
        raise ValueError("the planes must have one shape (n, H, W)")
    ow, oh = plane_reduced_size(w, h, d)
    out = {k: np.empty((n, oh, ow), dtype=PLANE_DTYPES[k]) for k in src}
    ptr = lambda arrs: [arrs[k].ctypes.data_as(_P) if k in arrs else None for k in PLANE_NAMES]
    _check(lib().dg_reduce_planes_host(w, h, n, ctypes.byref(d), *ptr(src), *ptr(out)))
    return out


def _depth_planes(n: int, height: int, width: int, distance: bool = True, kind: bool = True):
    """The two planes of n depth frames to fill, and the pointers to hand over (None for a plane that is not wanted)."""
    d = np.empty((n, height, width), dtype=np.int16) if distance else None
    k = np.empty((n, height, width), dtype=np.uint8) if kind else None
    return d, k, (d.ctypes.data_as(_P) if distance else None), (k.ctypes.data_as(_P) if kind else None)


def depth_lists_host(scene, width: int, height: int, frames, distance: bool = True, kind: bool = True):
    """dg_depth_lists_host: the depth planes of caller-built lists on the CPU (no ctx, no GPU); returns (int16 [n,H,W], uint8 [n,H,W]),
    None for a plane that was not asked for."""
    n = len(frames)
    d, k, dp, kp = _depth_planes(n, height, width, distance, kind)
    _check(lib().dg_depth_lists_host(scene._h, width, height, frames, n, dp, kp))
    return d, k


def owner_tag(cls: int, index: int) -> int:
    """The owner tag of a draw record: DG_LABEL_WALL or DG_LABEL_MOBJ << 16 | the seg's / map object's index."""
    return (cls << 16) | index


def owner_pointers(owners):
    """owners: per frame a uint32 array of owner tags (one per render record), or None -> (the `const uint32_t *const *` to hand over,
    keep-alive list)."""
    keep = [None if o is None else np.ascontiguousarray(o, dtype=np.uint32) for o in owners]
    arr = (_P * max(1, len(keep)))(*[None if o is None else o.ctypes.data_as(_P) for o in keep])
    return arr, keep


def _label_outputs(n: int, height: int, width: int, n_mobjs: int, id: bool = True, cls: bool = True, boxes: bool = True):
    """The planes and the box table of n label frames to fill, and the pointers to hand over (None for an output that is not wanted)."""
    i = np.empty((n, height, width), dtype=np.uint16) if id else None
    c = np.empty((n, height, width), dtype=np.uint8) if cls else None
    b = np.empty((n, n_mobjs), dtype=LABEL_BOX_DTYPE) if boxes else None
    return (i, c, b), [None if a is None else a.ctypes.data_as(_P) for a in (i, c, b)]


def label_lists_host(scene, width: int, height: int, frames, owners, id: bool = True, cls: bool = True, boxes: bool = True):
    """dg_label_lists_host: the label planes and boxes of caller-built lists on the CPU (no ctx, no GPU); owners: per frame the owner tags
    of its render records.  Returns (uint16 [n,H,W] id, uint8 [n,H,W] cls, LABEL_BOX_DTYPE [n, map objects]), None for what was not asked for."""
    n = len(frames)
    out, ptrs = _label_outputs(n, height, width, scene.mobj_count(), id, cls, boxes)
    op, keep = owner_pointers(owners)
    _check(lib().dg_label_lists_host(scene._h, width, height, frames, op, n, *ptrs))
    return out


def bundle_layout(width: int, height: int, n: int, what: int) -> dict:
    """dg_bundle_layout: the byte offsets of a bundle's parts in the slot's framebuffer slab (colour, distance, kind, id, cls) and `total`;
    a part not in `what` has offset == total.  No ctx, no GPU."""
    o = DgBundleOffsets()
    _check(lib().dg_bundle_layout(width, height, n, what, ctypes.byref(o)))
    return {k: getattr(o, k) for k, _ in o._fields_}


def bundle_lists_host(scene, width: int, height: int, frames, owners=None, distance: bool = True, kind: bool = True, id: bool = True, cls: bool = True,
                      boxes: bool = True):
    """dg_bundle_lists_host: the planes and boxes a bundle's fused kernel writes, for caller-built lists, on the CPU (no ctx, no GPU).
    owners (per frame the owner tags of its render records) is needed when id, cls or boxes is asked for.  Returns (distance, kind, id,
    cls, boxes) as depth_lists_host and label_lists_host give them, None for what was not asked for."""
    n = len(frames)
    d, k, dp, kp = _depth_planes(n, height, width, distance, kind)
    out, ptrs = _label_outputs(n, height, width, scene.mobj_count(), id, cls, boxes)
    op, keep = owner_pointers(owners) if owners is not None else (None, None)
    _check(lib().dg_bundle_lists_host(scene._h, width, height, frames, op, n, dp, kp, *ptrs))
    return (d, k) + tuple(out)


def seen_words(scene) -> int:
    """dg_seen_words: the uint32 words of one seen row of the scene (ceil(linedefs / 32))."""
    return _check(lib().dg_seen_words(scene._h))


def seen_lines_host(scene, id, cls) -> np.ndarray:
    """dg_seen_lines_host: the seen rows (n, words) uint32 of label planes id (n, H, W) uint16 and cls (n, H, W) uint8, on the CPU."""
    i = np.ascontiguousarray(id, dtype=np.uint16)
    c = np.ascontiguousarray(cls, dtype=np.uint8)
    if i.ndim != 3 or c.shape != i.shape:
        raise ValueError("id and cls must have one shape (n, H, W)")
    n, h, w = i.shape
    out = np.empty((n, seen_words(scene)), dtype=np.uint32)
    _check(lib().dg_seen_lines_host(scene._h, w, h, n, i.ctypes.data_as(_P), c.ctypes.data_as(_P), out.ctypes.data_as(_P)))
    return out


def _seen_outputs(count: int, runs: int, words: int, want):
    """The outputs of an accumulation to fill, {name: array} for the names in `want`, and the four pointers to hand over."""
    shapes = {"upto": (count, words), "total": (count,), "fresh": (count,), "carry_out": (runs, words)}
    out = {k: np.empty(shapes[k], dtype=np.uint32) for k in shapes if k in want}
    return out, [out[k].ctypes.data_as(_P) if k in out else None for k in shapes]


SEEN_OUTPUTS = ("upto", "total", "fresh", "carry_out")


def seen_accumulate_host(seen, run_len: int, carry_in=None, want=SEEN_OUTPUTS) -> dict:
    """dg_seen_accumulate_host: the running OR of the rows `seen` (n, words) along runs of run_len frames; carry_in (n / run_len, words)
    or None.  Returns {name: array} for the outputs named in `want` (upto, total, fresh, carry_out)."""
    sn = np.ascontiguousarray(seen, dtype=np.uint32)
    n, words = sn.shape
    ci = None if carry_in is None else np.ascontiguousarray(carry_in, dtype=np.uint32)
    out, ptrs = _seen_outputs(n, n // run_len if run_len > 0 else 0, words, want)
    _check(lib().dg_seen_accumulate_host(words, n, run_len, None if ci is None else ci.ctypes.data_as(_P), sn.ctypes.data_as(_P), *ptrs))
    return out


def explored_map_host(scene, width: int, height: int, view, mask_row) -> np.ndarray:
    """dg_explored_map_host: one explored map frame (H, W, 3) uint8 by the literal rule; view None: no arrow."""
    m = np.ascontiguousarray(mask_row, dtype=np.uint32)
    out = np.empty((height, width, 3), dtype=np.uint8)
    _check(lib().dg_explored_map_host(scene._h, width, height, ctypes.byref(view) if view is not None else None, m.ctypes.data_as(_P), out.ctypes.data_as(_P)))
    return out


def _ego_params(params) -> DgEgoMap:
    """A DgEgoMap as it is, or one from (scale, flags)."""
    return params if isinstance(params, DgEgoMap) else DgEgoMap(float(params[0]), int(params[1]))


def _mask_ptr(mask):
    """(keep-alive array, pointer) of mask rows, or (None, None)."""
    if mask is None:
        return None, None
    m = np.ascontiguousarray(mask, dtype=np.uint32)
    return m, m.ctypes.data_as(_P)


def ego_map_lines(scene, width: int, height: int, view, params) -> np.ndarray:
    """dg_ego_map_lines: the lines of one player-centred map frame in draw order, (n, 5) int64 rows [x0, y0, x1, y1, rgb]; params a
    DgEgoMap or (scale, flags)."""
    p = _ego_params(params)
    n = _check(lib().dg_ego_map_lines(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), None, 0))
    arr = (DgMapLine * max(1, n))()
    _check(lib().dg_ego_map_lines(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), arr, n))
    rows = np.frombuffer(arr, dtype=np.int32, count=5 * n).reshape(n, 5).astype(np.int64)
    rows[:, 4] &= 0xFFFFFFFF
    return rows


def ego_map_host(scene, width: int, height: int, view, params, mask_row=None) -> np.ndarray:
    """dg_ego_map_host: one player-centred map frame (H, W, 3) uint8 by the literal rule; mask_row None: every line."""
    p = _ego_params(params)
    _keep, mp = _mask_ptr(mask_row)
    out = np.empty((height, width, 3), dtype=np.uint8)
    _check(lib().dg_ego_map_host(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), mp, out.ctypes.data_as(_P)))
    return out


def floor_map_host(scene, width: int, height: int, view, params, mask_row=None, state=None, surfaces=None, out=None) -> np.ndarray:
    """dg_floor_map_host: one floor-textured player-centred map frame (H, W, 3) uint8 by the literal rule; mask_row None: every line and
    every sector; state a (lights, mobjs) pair and surfaces a (sides, flats) pair as make_view_states / make_view_surfaces take them, or
    None.  out: the array to fill (else a new one)."""
    p = _ego_params(params)
    _keep, mp = _mask_ptr(mask_row)
    vs, _keep2 = make_view_states([state]) if state is not None else (None, None)
    vf, _keep3 = make_view_surfaces([surfaces]) if surfaces is not None else (None, None)
    if out is None:
        out = np.empty((height, width, 3), dtype=np.uint8)
    _check(lib().dg_floor_map_host(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), mp, vs, vf, out.ctypes.data_as(_P)))
    return out


def _one_view_inputs(state, poses, surfaces=None):
    """(dg_view_state *, dg_view_poses *, dg_view_surfaces *, keep-alive) of ONE view's inputs, each None or as make_view_* takes an entry."""
    vs, k1 = make_view_states([state]) if state is not None else (None, None)
    vp, k2 = make_view_poses([poses]) if poses is not None else (None, None)
    vf, k3 = make_view_surfaces([surfaces]) if surfaces is not None else (None, None)
    return vs, vp, vf, (k1, k2, k3)


def map_thing_lines(scene, width: int, height: int, view, params, state=None, poses=None) -> np.ndarray:
    """dg_map_thing_lines: the marker lines of one map frame in draw order, (n, 5) int64 rows [x0, y0, x1, y1, rgb]; state a (lights, mobjs)
    pair and poses a list of (mobj, x, y, angle) entries, or None."""
    p = _ego_params(params)
    vs, vp, _, _keep = _one_view_inputs(state, poses)
    n = _check(lib().dg_map_thing_lines(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), vs, vp, None, 0))
    arr = (DgMapLine * max(1, n))()
    _check(lib().dg_map_thing_lines(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), vs, vp, arr, n))
    rows = np.frombuffer(arr, dtype=np.int32, count=5 * n).reshape(n, 5).astype(np.int64)
    rows[:, 4] &= 0xFFFFFFFF
    return rows


def ego_map_things_host(scene, width: int, height: int, view, params, mask_row=None, state=None, poses=None) -> np.ndarray:
    """dg_ego_map_things_host: one player-centred map frame with the map objects' markers (H, W, 3) uint8 by the literal rule."""
    p = _ego_params(params)
    _keep, mp = _mask_ptr(mask_row)
    vs, vp, _, _keep2 = _one_view_inputs(state, poses)
    out = np.empty((height, width, 3), dtype=np.uint8)
    _check(lib().dg_ego_map_things_host(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), mp, vs, vp, out.ctypes.data_as(_P)))
    return out


def floor_map_things_host(scene, width: int, height: int, view, params, mask_row=None, state=None, surfaces=None, poses=None) -> np.ndarray:
    """dg_floor_map_things_host: one floor-textured map frame with the map objects' markers (H, W, 3) uint8 by the literal rule."""
    p = _ego_params(params)
    _keep, mp = _mask_ptr(mask_row)
    vs, vp, vf, _keep2 = _one_view_inputs(state, poses, surfaces)
    out = np.empty((height, width, 3), dtype=np.uint8)
    _check(lib().dg_floor_map_things_host(scene._h, width, height, ctypes.byref(view), ctypes.byref(p), mp, vs, vf, vp, out.ctypes.data_as(_P)))
    return out


# a dg_sight_query as numpy sees it (dg_sight_host, dg_sight_device)
SIGHT_QUERY_DTYPE = np.dtype([("frame", "<i4"), ("x0", "<f4"), ("y0", "<f4"), ("z0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("z1_lo", "<f4"), ("z1_hi", "<f4")])


def _sight_queries(queries) -> np.ndarray:
    q = np.ascontiguousarray(queries, dtype=SIGHT_QUERY_DTYPE).reshape(-1)
    return q


def _sight_mobj_args(scene, views, mobj_height):
    n_mobjs = lib().dg_scene_mobj_count(scene._h)
    heights = np.ascontiguousarray(mobj_height, dtype=np.float32).reshape(-1)
    if heights.size != n_mobjs:
        raise ValueError("mobj_height must hold one height per map object")
    words = _check(lib().dg_sight_words(scene._h))
    return heights, np.empty((len(views), words), dtype=np.uint32)


def sight_host(scene, queries, sectors=None, n_frames: int = 1) -> np.ndarray:
    """dg_sight_host: one byte per query (SIGHT_QUERY_DTYPE array), 1 visible, 0 not; sectors: make_view_sectors' array of n_frames
    elements, or None (every frame has the scene's heights)."""
    q = _sight_queries(queries)
    out = np.empty(q.size, dtype=np.uint8)
    _check(lib().dg_sight_host(scene._h, sectors, n_frames, q.ctypes.data_as(_P), q.size, out.ctypes.data_as(_P)))
    return out


def sight_mobjs_host(scene, views, eye_height: float, mobj_height, poses=None, sectors=None) -> np.ndarray:
    """dg_sight_mobjs_host: which map objects every view sees, a (len(views), dg_sight_words) uint32 array of bit rows.  mobj_height: one
    float per map object (<= 0 leaves it out); poses / sectors: make_view_poses' / make_view_sectors' arrays, or None."""
    heights, out = _sight_mobj_args(scene, views, mobj_height)
    _check(lib().dg_sight_mobjs_host(scene._h, views, poses, sectors, len(views), eye_height, heights.ctypes.data_as(_P), out.ctypes.data_as(_P)))
    return out


def make_view_states(states):
    """states: one (lights, mobjs) pair per view; lights = [(sector, light_level), ...], mobjs = [(mobj, sprite_frame or -1, full_bright), ...].
    Returns (ctypes array of dg_view_state, keep-alive list)."""
    arr = (DgViewState * len(states))()
    keep = []
    for i, (lights, mobjs) in enumerate(states):
        la = (DgSectorLight * max(1, len(lights)))(*[DgSectorLight(int(s), int(l)) for s, l in lights])
        ma = (DgMobjState * max(1, len(mobjs)))(*[DgMobjState(int(m), int(sf), int(fb), 0) for m, sf, fb in mobjs])
        keep += [la, ma]
        arr[i] = DgViewState(la, len(lights), ma, len(mobjs))
    return arr, keep


def make_view_poses(poses):
    """poses: one list per view of (mobj, x, y, angle) entries (dg_mobj_pose; the floats are taken as float32).
    Returns (ctypes array of dg_view_poses, keep-alive list)."""
    arr = (DgViewPoses * max(1, len(poses)))()
    keep = []
    for i, entries in enumerate(poses):
        pa = (DgMobjPose * max(1, len(entries)))(*[DgMobjPose(int(m), float(x), float(y), float(a)) for m, x, y, a in entries])
        keep.append(pa)
        arr[i] = DgViewPoses(pa, len(entries))
    return arr, keep


def make_view_sectors(sectors):
    """sectors: one list per view of (sector, floor_height, ceiling_height) entries (dg_sector_heights).
    Returns (ctypes array of dg_view_sectors, keep-alive list)."""
    arr = (DgViewSectors * max(1, len(sectors)))()
    keep = []
    for i, entries in enumerate(sectors):
        ha = (DgSectorHeights * max(1, len(entries)))(*[DgSectorHeights(int(s), int(f), int(c)) for s, f, c in entries])
        keep.append(ha)
        arr[i] = DgViewSectors(ha, len(entries))
    return arr, keep


def make_view_surfaces(surfaces):
    """surfaces: one (sides, flats) pair per view — sides a list of (sidedef, tex_mid, tex_low, tex_up, x_offset, y_offset) entries
    (dg_side_surface), flats a list of (sector, floor_flat, ceil_flat) entries (dg_sector_flats).
    Returns (ctypes array of dg_view_surfaces, keep-alive list)."""
    arr = (DgViewSurfaces * max(1, len(surfaces)))()
    keep = []
    for i, (sides, flats) in enumerate(surfaces):
        sa = (DgSideSurface * max(1, len(sides)))(*[DgSideSurface(*[int(v) for v in e]) for e in sides])
        fa = (DgSectorFlats * max(1, len(flats)))(*[DgSectorFlats(*[int(v) for v in e]) for e in flats])
        keep += [sa, fa]
        arr[i] = DgViewSurfaces(sa, len(sides), fa, len(flats))
    return arr, keep


def make_views(records, timestamp: float = 0.0):
    """camera_path records (n, 8) f32 [x, y, angle, cos, sin, cos(-a), sin(-a), floor] -> ctypes array of dg_view."""
    recs = np.asarray(records, dtype=np.float32).reshape(-1, 8)
    arr = (DgView * len(recs))()
    for i, r in enumerate(recs):
        arr[i] = DgView(float(r[0]), float(r[1]), float(r[2]), float(r[7]), float(r[3]), float(r[4]), float(r[5]), float(r[6]),
                        float(timestamp), 1)
    return arr


class Scene:
    """dg_scene: Map + Palette + Textures + Flats + Sprites + MapObjects of one map (src/game.rs:142-167)."""

    def __init__(self, wad: bytes, map_name: str = "e1m1"):
        h = _P()
        _check(lib().dg_scene_load_wad(wad, len(wad), map_name.encode(), ctypes.byref(h)))
        self._h = h

    def player_start(self):
        x, y, a = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(lib().dg_scene_player_start(self._h, x, y, a))
        return x.value, y.value, a.value

    def floor_height_at(self, x: float, y: float, default: float = 0.0) -> float:
        h = ctypes.c_float(default)
        _check(lib().dg_scene_floor_height_at(self._h, x, y, h))
        return h.value

    def sector_count(self) -> int:
        return lib().dg_scene_sector_count(self._h)

    def set_sector_light(self, sector: int, light: int):
        _check(lib().dg_scene_set_sector_light(self._h, sector, light))

    def mobj_count(self) -> int:
        return lib().dg_scene_mobj_count(self._h)

    def sprite_frame(self, sprite: str, frame: int = 0) -> int:
        """Handle for dg_mobj_state.sprite_frame (may decode bitmaps: call before Context.upload_scene)."""
        return _check(lib().dg_scene_sprite_frame(self._h, sprite.encode(), frame))

    def set_mobj_state(self, mobj: int, sprite, frame: int = 0, full_bright: bool = False):
        _check(lib().dg_scene_set_mobj_state(self._h, mobj, sprite.encode() if sprite else None, frame, int(full_bright)))

    def set_map_markers(self, markers):
        """dg_scene_set_map_markers: one (radius, rgb, flags) per map object (rgb r | g << 8 | b << 16, flags DG_MARK_BOX | DG_MARK_HEADING or 0),
        or None: no table.  The host functions see it at once, a Context at upload_scene."""
        if markers is None:
            _check(lib().dg_scene_set_map_markers(self._h, None, 0))
            return
        arr = (DgMapMarker * max(1, len(markers)))(*[DgMapMarker(int(r), int(c), int(f)) for r, c, f in markers])
        _check(lib().dg_scene_set_map_markers(self._h, arr, len(markers)))

    def set_wall_effects(self, flags: int):
        """dg_scene_set_wall_effects: DG_WALL_ANIMATE | DG_WALL_SCROLL, or 0 (may decode bitmaps: call before Context.upload_scene,
        which is where the flags take effect for a Context; build_lists sees them at once)."""
        _check(lib().dg_scene_set_wall_effects(self._h, flags))

    def wall_texture_id(self, name: str, timestamp: float = 0.0) -> int:
        """dg_scene_wall_texture_id: the texture's bitmap id after wall animation at `timestamp` (negative: unknown)."""
        return lib().dg_scene_wall_texture_id(self._h, name.encode(), timestamp)

    def set_light_effects(self, flags: int, seed: int = 0):
        """dg_scene_set_light_effects: DG_LIGHT_THINKERS or 0, and the seed of the random effects' stream (takes effect for a Context
        at Context.upload_scene; build_lists and sector_lights_at see it at once)."""
        _check(lib().dg_scene_set_light_effects(self._h, flags, seed & 0xFFFFFFFFFFFFFFFF))

    def sector_lights_at(self, timestamp: float):
        """dg_scene_sector_lights_at: every sector's level at `timestamp` as drawn with no view state (numpy int16 array)."""
        n = lib().dg_scene_sector_count(self._h)
        out = np.zeros(max(n, 0), dtype=np.int16)
        _check(lib().dg_scene_sector_lights_at(self._h, timestamp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n))
        return out

    def set_mobj_thinkers(self, flags: int, states=(), infos=()):
        """dg_scene_set_mobj_thinkers: DG_MOBJ_THINKERS or 0; states = [(sprite, frame, full_bright, tics, next_state), ...] with row 0
        S_NULL, infos = [(doomednum, spawn_state, death_state, xdeath_state), ...] (takes effect for a Context at Context.upload_scene;
        build_lists and mobj_states_at see it at once).  Drops the event list."""
        sa = (DgStateRec * max(1, len(states)))(*[DgStateRec((sp or "").encode(), int(fr), int(bool(fb)), int(tics), int(nxt))
                                                  for sp, fr, fb, tics, nxt in states])
        ia = (DgMobjInfoRec * max(1, len(infos)))(*[DgMobjInfoRec(*[int(v) for v in row]) for row in infos])
        _check(lib().dg_scene_set_mobj_thinkers(self._h, flags, sa, len(states), ia, len(infos)))

    def mobj_event(self, what: int, timestamp: float = 0.0):
        """dg_scene_mobj_event: DG_MOBJ_KILL / _EXPLODE / _RESPAWN for every map object at `timestamp`; 0 clears the list."""
        _check(lib().dg_scene_mobj_event(self._h, what, timestamp))

    def mobj_states_at(self, timestamp: float):
        """dg_scene_mobj_states_at: every map object's (sprite_frame or -1, full_bright) at `timestamp` as drawn with no view state."""
        n = lib().dg_scene_mobj_count(self._h)
        out = (DgMobjState * max(1, n))()
        _check(lib().dg_scene_mobj_states_at(self._h, timestamp, out, n))
        return [(out[i].sprite_frame, out[i].full_bright) for i in range(n)]

    def build_lists(self, W: int, H: int, view: DgView) -> DgFrameLists:
        fl = DgFrameLists()
        _check(lib().dg_build_lists(self._h, W, H, ctypes.byref(view), ctypes.byref(fl)))
        return fl

    def build_lists_owners(self, W: int, H: int, view: DgView):
        """dg_build_lists_owners: the lists of dg_build_lists and, as a uint32 array of its own, the owner tag of every render record."""
        fl = DgFrameLists()
        own = ctypes.POINTER(ctypes.c_uint32)()
        _check(lib().dg_build_lists_owners(self._h, W, H, ctypes.byref(view), ctypes.byref(fl), ctypes.byref(own)))
        return fl, np.array(own[:fl.n_renders], dtype=np.uint32)

    def build_lists_poses(self, W: int, H: int, view: DgView, poses=None, owners: bool = False):
        """dg_build_lists_poses: dg_build_lists for a view whose map objects stand where `poses` says ([(mobj, x, y, angle), ...] or
        None); with owners=True returns (lists, owner tags) as build_lists_owners does."""
        fl = DgFrameLists()
        vp, _keep = make_view_poses([poses]) if poses is not None else (None, None)
        own = ctypes.POINTER(ctypes.c_uint32)()
        _check(lib().dg_build_lists_poses(self._h, W, H, ctypes.byref(view), vp, ctypes.byref(fl), ctypes.byref(own) if owners else None))
        return (fl, np.array(own[:fl.n_renders], dtype=np.uint32)) if owners else fl

    def build_lists_sectors(self, W: int, H: int, view: DgView, sectors=None, poses=None, owners: bool = False):
        """dg_build_lists_sectors: build_lists_poses for a view whose sectors have the heights `sectors` says
        ([(sector, floor, ceiling), ...] or None)."""
        fl = DgFrameLists()
        vp, _keep = make_view_poses([poses]) if poses is not None else (None, None)
        vs, _keep2 = make_view_sectors([sectors]) if sectors is not None else (None, None)
        own = ctypes.POINTER(ctypes.c_uint32)()
        _check(lib().dg_build_lists_sectors(self._h, W, H, ctypes.byref(view), vp, vs, ctypes.byref(fl), ctypes.byref(own) if owners else None))
        return (fl, np.array(own[:fl.n_renders], dtype=np.uint32)) if owners else fl

    def build_lists_surfaces(self, W: int, H: int, view: DgView, surfaces=None, sectors=None, poses=None, owners: bool = False):
        """dg_build_lists_surfaces: build_lists_sectors for a view whose sidedefs and flats are what `surfaces` says
        ((sides, flats) as make_view_surfaces takes them, or None)."""
        fl = DgFrameLists()
        vp, _keep = make_view_poses([poses]) if poses is not None else (None, None)
        vs, _keep2 = make_view_sectors([sectors]) if sectors is not None else (None, None)
        vf, _keep3 = make_view_surfaces([surfaces]) if surfaces is not None else (None, None)
        own = ctypes.POINTER(ctypes.c_uint32)()
        _check(lib().dg_build_lists_surfaces(self._h, W, H, ctypes.byref(view), vp, vs, vf, ctypes.byref(fl), ctypes.byref(own) if owners else None))
        return (fl, np.array(own[:fl.n_renders], dtype=np.uint32)) if owners else fl

    def use_texture(self, name: str) -> int:
        """dg_scene_use_texture: the bitmap id of the wall texture `name` (TEX_NONE for "-"), decoded now if the map did not use it.
        Call before Context.upload_scene."""
        return _check(lib().dg_scene_use_texture(self._h, name.encode())) if name != "-" else TEX_NONE

    def use_flat(self, name: str) -> int:
        """dg_scene_use_flat: a flat handle for `name`, its lump (or its whole animated list) loaded now if the map did not use it.
        Call before Context.upload_scene."""
        return _check(lib().dg_scene_use_flat(self._h, name.encode()))

    def use_picture(self, name: str) -> int:
        """dg_scene_use_picture: the handle of the picture lump `name` (a sprite lump, a patch, any lump in picture format), decoded now
        if the scene does not hold it.  Call before Context.upload_scene."""
        return _check(lib().dg_scene_use_picture(self._h, name.encode()))

    def picture_count(self) -> int:
        return _check(lib().dg_scene_picture_count(self._h))

    def picture_info(self, picture: int):
        """dg_scene_picture_info: (w, h, left_offset, top_offset) of a picture handle."""
        v = [ctypes.c_int32() for _ in range(4)]
        _check(lib().dg_scene_picture_info(self._h, picture, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def sidedef_count(self) -> int:
        return _check(lib().dg_scene_sidedef_count(self._h))

    def sidedef_surfaces(self) -> np.ndarray:
        """dg_scene_sidedef_surfaces: every sidedef as loaded, an (n, 6) int32 array [sidedef, tex_mid, tex_low, tex_up, x_offset, y_offset]."""
        n = self.sidedef_count()
        out = np.zeros((max(n, 0), 6), dtype=np.int32)
        _check(lib().dg_scene_sidedef_surfaces(self._h, out.ctypes.data_as(ctypes.POINTER(DgSideSurface)), n))
        return out

    def sector_flats(self) -> np.ndarray:
        """dg_scene_sector_flats: every sector's flat handles as loaded, an (n, 3) int32 array [sector, floor_flat, ceil_flat]."""
        n = lib().dg_scene_sector_count(self._h)
        out = np.zeros((max(n, 0), 3), dtype=np.int32)
        _check(lib().dg_scene_sector_flats(self._h, out.ctypes.data_as(ctypes.POINTER(DgSectorFlats)), n))
        return out

    def sector_heights(self) -> np.ndarray:
        """dg_scene_sector_heights: every sector's (floor, ceiling) as loaded, an (n, 2) int16 array."""
        n = lib().dg_scene_sector_count(self._h)
        fl = np.zeros(max(n, 0), dtype=np.int16)
        ce = np.zeros(max(n, 0), dtype=np.int16)
        _check(lib().dg_scene_sector_heights(self._h, fl.ctypes.data_as(_P), ce.ctypes.data_as(_P), n))
        return np.stack([fl, ce], axis=1)

    def sectors_at(self, x, y) -> np.ndarray:
        """dg_scene_sectors_at: get_sector_from_vertex of every point (float32 arrays x, y) as an int32 array, -1 for None."""
        xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        ys = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
        if xs.size != ys.size:
            raise ValueError("x and y differ in length")
        out = np.empty(xs.size, dtype=np.int32)
        _check(lib().dg_scene_sectors_at(self._h, xs.ctypes.data_as(_P), ys.ctypes.data_as(_P), xs.size, out.ctypes.data_as(_P)))
        return out

    def mobj_poses(self) -> np.ndarray:
        """dg_scene_mobj_poses: every map object's pose and sector as loaded (MOBJ_PLACED_DTYPE array)."""
        n = lib().dg_scene_mobj_count(self._h)
        out = np.zeros(max(n, 0), dtype=MOBJ_PLACED_DTYPE)
        _check(lib().dg_scene_mobj_poses(self._h, out.ctypes.data_as(_P), n))
        return out

    def bsp_depth(self) -> int:
        """dg_scene_bsp_depth: the nodes on the longest way from the BSP's root to a leaf."""
        return _check(lib().dg_scene_bsp_depth(self._h))

    def map_lines(self, W: int, H: int, view=None) -> np.ndarray:
        """dg_map_lines: the lines of one 2-D map frame in draw order, (n, 5) int64 rows [x0, y0, x1, y1, rgb] (rgb = r | g<<8 | b<<16);
        view None: the linedefs only."""
        vp = ctypes.byref(view) if view is not None else None
        n = _check(lib().dg_map_lines(self._h, W, H, vp, None, 0))
        arr = (DgMapLine * max(1, n))()
        _check(lib().dg_map_lines(self._h, W, H, vp, arr, n))
        rows = np.frombuffer(arr, dtype=np.int32, count=5 * n).reshape(n, 5).astype(np.int64)
        rows[:, 4] &= 0xFFFFFFFF
        return rows

    def close(self):
        if self._h:
            lib().dg_scene_free(self._h)
            self._h = None


class Walk:
    """dg_walk: a play-through moved as the reference moves its player (Game::process_down_keys, src/game.rs:314-389): a start pose
    (x, y, angle; None: Player1Start), --turbo in percent and one DG_KEY_* mask per 35 Hz tic.  floors() / views() find the floor
    heights on the host unless Context.locate_walks has found them on the GPU.  The scene must outlive the walk."""

    def __init__(self, scene: Scene, keys, start=None, turbo: int = 100):
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        x, y, a = (0.0, 0.0, 0.0) if start is None else start
        d = DgWalkDesc(x, y, a, int(start is None), int(turbo), k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if k.size else None, k.size)
        h = _P()
        _check(lib().dg_walk_create(scene._h, ctypes.byref(d), ctypes.byref(h)))
        self._h = h
        self._scene = scene  # keep alive

    def tics(self) -> int:
        return _check(lib().dg_walk_tics(self._h))

    def probe_count(self) -> int:
        return _check(lib().dg_walk_probe_count(self._h))

    def floors(self) -> np.ndarray:
        """dg_walk_floors: floor_height after 0 .. tics() tics (float32 array)."""
        out = np.zeros(self.tics() + 1, dtype=np.float32)
        _check(lib().dg_walk_floors(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size))
        return out

    def views(self, timestamps):
        """dg_walk_views: a ctypes array of dg_view, one per timestamp, for every submit / render / map call."""
        ts = np.ascontiguousarray(timestamps, dtype=np.float32).reshape(-1)
        arr = (DgView * max(1, ts.size))()
        _check(lib().dg_walk_views(self._h, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ts.size, arr))
        return arr if ts.size else (DgView * 0)()

    def close(self):
        if self._h:
            lib().dg_walk_free(self._h)
            self._h = None


class Context:
    """dg_ctx on one GPU.  Mirrors the reference call shape: for every view, `Pixels::new()` +
    `Renderer::new(..).render()` -> `pixels.pixels` (src/game.rs:505-525), batched."""

    def __init__(self, width: int, height: int, max_batch: int = 64, slots: int = 2, device: int = 0, host_threads: int = 0,
                 front_end: int = 0):
        cfg = DgConfig(device, width, height, max_batch, slots, host_threads, front_end)
        h = _P()
        _check(lib().dg_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.width, self.height, self.max_batch, self.slots = width, height, max_batch, slots
        self.frame_bytes = 3 * width * height
        self.host_threads = lib().dg_ctx_host_threads(self._h)
        self._scene = None

    def upload_scene(self, scene: Scene):
        _check(lib().dg_upload_scene(self._h, scene._h))
        self._scene = scene  # keep alive

    def render(self, views) -> np.ndarray:
        """Synchronous full path; returns (n, H, W, 3) uint8."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_views(self._h, views, n, out.ctypes.data_as(_P)))
        return out

    def render_one_into(self, view: DgView, host_ptr: int):
        """`Renderer::new(..).render()` for ONE view, synchronously, RGB24 written to caller memory (the drop-in call shape:
        rust/src/gpu.rs GpuRenderer::render)."""
        _check(lib().dg_render_views(self._h, ctypes.byref(view), 1, _P(host_ptr)))

    def submit(self, slot: int, views, n=None, states=None):
        if states is None:
            _check(lib().dg_submit_views(self._h, slot, views, len(views) if n is None else n))
        else:
            _check(lib().dg_submit_views_state(self._h, slot, views, states, len(views) if n is None else n))

    def submit_poses(self, slot: int, views, poses, n=None, states=None):
        """dg_submit_views_poses: submit() with a dg_view_poses per view (make_view_poses; None: none)."""
        _check(lib().dg_submit_views_poses(self._h, slot, views, states, poses, len(views) if n is None else n))

    def render_poses(self, views, poses, states=None) -> np.ndarray:
        """dg_render_views_poses: synchronous, slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_views_poses(self._h, views, states, poses, n, out.ctypes.data_as(_P)))
        return out

    def submit_bundle_poses(self, slot: int, views, what: int, poses, n=None, states=None):
        """dg_submit_bundle_views_poses: submit_bundle() with a dg_view_poses per view."""
        _check(lib().dg_submit_bundle_views_poses(self._h, slot, views, states, poses, len(views) if n is None else n, what))

    def slot_mobj_poses(self, slot: int, first: int, count: int) -> np.ndarray:
        """dg_slot_mobj_poses: the pose rows (count, map objects) of MOBJ_PLACED_DTYPE the slot's frames were drawn with."""
        n = lib().dg_scene_mobj_count(self._scene._h) if self._scene is not None else 0
        out = np.zeros((max(count, 0), max(n, 0)), dtype=MOBJ_PLACED_DTYPE)
        _check(lib().dg_slot_mobj_poses(self._h, slot, first, count, out.ctypes.data_as(_P)))
        return out

    def mobj_pose_timing(self, slot: int) -> float:
        """dg_slot_mobj_pose_timing: GPU time (ms) of the pose kernels of the slot's last submission (0: none ran)."""
        t = ctypes.c_float()
        _check(lib().dg_slot_mobj_pose_timing(self._h, slot, ctypes.byref(t)))
        return t.value

    def submit_sectors(self, slot: int, views, sectors, n=None, states=None, poses=None):
        """dg_submit_views_sectors: submit_poses() with a dg_view_sectors per view (make_view_sectors; None: none)."""
        _check(lib().dg_submit_views_sectors(self._h, slot, views, states, poses, sectors, len(views) if n is None else n))

    def render_sectors(self, views, sectors, states=None, poses=None) -> np.ndarray:
        """dg_render_views_sectors: synchronous, slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_views_sectors(self._h, views, states, poses, sectors, n, out.ctypes.data_as(_P)))
        return out

    def submit_bundle_sectors(self, slot: int, views, what: int, sectors, n=None, states=None, poses=None):
        """dg_submit_bundle_views_sectors: submit_bundle_poses() with a dg_view_sectors per view."""
        _check(lib().dg_submit_bundle_views_sectors(self._h, slot, views, states, poses, sectors, len(views) if n is None else n, what))

    def slot_sector_heights(self, slot: int, first: int, count: int) -> np.ndarray:
        """dg_slot_sector_heights: the (count, sectors, 2) int16 heights (floor, ceiling) the slot's frames were drawn with."""
        n = lib().dg_scene_sector_count(self._scene._h) if self._scene is not None else 0
        out = np.zeros((max(count, 0), max(n, 0), 2), dtype=np.int16)
        _check(lib().dg_slot_sector_heights(self._h, slot, first, count, out.ctypes.data_as(_P)))
        return out

    def sector_height_timing(self, slot: int) -> float:
        """dg_slot_sector_height_timing: GPU time (ms) of the row kernels of the slot's last submission (0: none ran)."""
        t = ctypes.c_float()
        _check(lib().dg_slot_sector_height_timing(self._h, slot, ctypes.byref(t)))
        return t.value

    def submit_surfaces(self, slot: int, views, surfaces, n=None, states=None, poses=None, sectors=None):
        """dg_submit_views_surfaces: submit_sectors() with a dg_view_surfaces per view (make_view_surfaces; None: none)."""
        _check(lib().dg_submit_views_surfaces(self._h, slot, views, states, poses, sectors, surfaces, len(views) if n is None else n))

    def render_surfaces(self, views, surfaces, states=None, poses=None, sectors=None) -> np.ndarray:
        """dg_render_views_surfaces: synchronous, slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_views_surfaces(self._h, views, states, poses, sectors, surfaces, n, out.ctypes.data_as(_P)))
        return out

    def submit_bundle_surfaces(self, slot: int, views, what: int, surfaces, n=None, states=None, poses=None, sectors=None):
        """dg_submit_bundle_views_surfaces: submit_bundle_sectors() with a dg_view_surfaces per view."""
        _check(lib().dg_submit_bundle_views_surfaces(self._h, slot, views, states, poses, sectors, surfaces, len(views) if n is None else n, what))

    def slot_sector_flats(self, slot: int, first: int, count: int) -> np.ndarray:
        """dg_slot_sector_flats: the (count, sectors, 2) int32 flat handles (floor, ceiling) the slot's frames were drawn with."""
        n = lib().dg_scene_sector_count(self._scene._h) if self._scene is not None else 0
        out = np.zeros((max(count, 0), max(n, 0), 2), dtype=np.int32)
        _check(lib().dg_slot_sector_flats(self._h, slot, first, count, out.ctypes.data_as(_P)))
        return out

    def surface_timing(self, slot: int) -> float:
        """dg_slot_surface_timing: GPU time (ms) of the flat row kernels of the slot's last submission (0: none ran)."""
        t = ctypes.c_float()
        _check(lib().dg_slot_surface_timing(self._h, slot, ctypes.byref(t)))
        return t.value

    def submit_map(self, slot: int, views, n=None):
        """dg_submit_map_views: 2-D map frames (the reference's viewing_map) into the slot, asynchronously."""
        _check(lib().dg_submit_map_views(self._h, slot, views, len(views) if n is None else n))

    def render_map(self, views) -> np.ndarray:
        """dg_render_map_views: synchronous 2-D map frames through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_map_views(self._h, views, n, out.ctypes.data_as(_P)))
        return out

    def submit_explored_map(self, slot: int, views, mask, n=None):
        """dg_submit_explored_map_views: map frames that show only the linedefs whose bit is set in mask (n, words) uint32, asynchronously."""
        m = np.ascontiguousarray(mask, dtype=np.uint32)
        _check(lib().dg_submit_explored_map_views(self._h, slot, views, len(views) if n is None else n, m.ctypes.data_as(_P)))

    def render_explored_map(self, views, mask) -> np.ndarray:
        """dg_render_explored_map_views: synchronous through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        m = np.ascontiguousarray(mask, dtype=np.uint32)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_explored_map_views(self._h, views, n, m.ctypes.data_as(_P), out.ctypes.data_as(_P)))
        return out

    def submit_ego_map(self, slot: int, views, params, mask=None, n=None):
        """dg_submit_ego_map_views: player-centred map frames (params a DgEgoMap or (scale, flags); mask (n, words) uint32 or None: every
        line), asynchronously."""
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        _check(lib().dg_submit_ego_map_views(self._h, slot, views, len(views) if n is None else n, ctypes.byref(p), mp))

    def render_ego_map(self, views, params, mask=None) -> np.ndarray:
        """dg_render_ego_map_views: synchronous through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_ego_map_views(self._h, views, n, ctypes.byref(p), mp, out.ctypes.data_as(_P)))
        return out

    def submit_floor_map(self, slot: int, views, params, mask=None, states=None, surfaces=None, n=None):
        """dg_submit_floor_map_views: floor-textured player-centred map frames (params and mask as submit_ego_map; states / surfaces:
        one entry per view as make_view_states / make_view_surfaces take them, or None), asynchronously."""
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vf, _keep3 = make_view_surfaces(surfaces) if surfaces is not None else (None, None)
        _check(lib().dg_submit_floor_map_views(self._h, slot, views, len(views) if n is None else n, ctypes.byref(p), mp, vs, vf))

    def render_floor_map(self, views, params, mask=None, states=None, surfaces=None) -> np.ndarray:
        """dg_render_floor_map_views: synchronous through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vf, _keep3 = make_view_surfaces(surfaces) if surfaces is not None else (None, None)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_floor_map_views(self._h, views, n, ctypes.byref(p), mp, vs, vf, out.ctypes.data_as(_P)))
        return out

    def submit_ego_map_things(self, slot: int, views, params, mask=None, states=None, poses=None, n=None):
        """dg_submit_ego_map_views_things: submit_ego_map with the map objects' markers (states / poses: one entry per view as
        make_view_states / make_view_poses take them, or None), asynchronously."""
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vp, _keep3 = make_view_poses(poses) if poses is not None else (None, None)
        _check(lib().dg_submit_ego_map_views_things(self._h, slot, views, len(views) if n is None else n, ctypes.byref(p), mp, vs, vp))

    def render_ego_map_things(self, views, params, mask=None, states=None, poses=None) -> np.ndarray:
        """dg_render_ego_map_views_things: synchronous through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vp, _keep3 = make_view_poses(poses) if poses is not None else (None, None)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_ego_map_views_things(self._h, views, n, ctypes.byref(p), mp, vs, vp, out.ctypes.data_as(_P)))
        return out

    def submit_floor_map_things(self, slot: int, views, params, mask=None, states=None, surfaces=None, poses=None, n=None):
        """dg_submit_floor_map_views_things: submit_floor_map with the map objects' markers, asynchronously."""
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vf, _keep3 = make_view_surfaces(surfaces) if surfaces is not None else (None, None)
        vp, _keep4 = make_view_poses(poses) if poses is not None else (None, None)
        _check(lib().dg_submit_floor_map_views_things(self._h, slot, views, len(views) if n is None else n, ctypes.byref(p), mp, vs, vf, vp))

    def render_floor_map_things(self, views, params, mask=None, states=None, surfaces=None, poses=None) -> np.ndarray:
        """dg_render_floor_map_views_things: synchronous through slot 0; returns (n, H, W, 3) uint8."""
        n = len(views)
        p = _ego_params(params)
        _keep, mp = _mask_ptr(mask)
        vs, _keep2 = make_view_states(states) if states is not None else (None, None)
        vf, _keep3 = make_view_surfaces(surfaces) if surfaces is not None else (None, None)
        vp, _keep4 = make_view_poses(poses) if poses is not None else (None, None)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_floor_map_views_things(self._h, views, n, ctypes.byref(p), mp, vs, vf, vp, out.ctypes.data_as(_P)))
        return out

    def seen_lines_device(self, width: int, height: int, n_frames: int, id_ptr: int, cls_ptr: int, seen_ptr: int):
        """dg_seen_lines_device: the seen rows of n_frames label planes at the device addresses id_ptr / cls_ptr into device address seen_ptr
        (synchronous; planes of a finished slot's framebuffer_ptr or tensors' data_ptr()).  Touches no slot."""
        _check(lib().dg_seen_lines_device(self._h, width, height, n_frames, _P(id_ptr), _P(cls_ptr), _P(seen_ptr)))

    def slot_seen_lines(self, slot: int, first: int, count: int, run_len: int, carry_in=None, want=SEEN_OUTPUTS) -> dict:
        """dg_slot_seen_lines: the seen rows of frames [first, first + count) of a label slot (or a bundle slot with labels), accumulated along
        runs of run_len frames; carry_in (count / run_len, words) or None.  Returns {name: array} for the outputs named in `want`."""
        words = seen_words(self._scene)
        ci = None if carry_in is None else np.ascontiguousarray(carry_in, dtype=np.uint32)
        out, ptrs = _seen_outputs(count, count // run_len if run_len > 0 else 0, words, want)
        _check(lib().dg_slot_seen_lines(self._h, slot, first, count, run_len, None if ci is None else ci.ctypes.data_as(_P), *ptrs))
        return out

    def seen_kernel_ms(self) -> dict:
        """dg_ctx_seen_kernel_ms: GPU time (ms) of the last seen_lines_device / slot_seen_lines call's kernels."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().dg_ctx_seen_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"lines_ms": a.value, "accumulate_ms": b.value}

    def sight(self, queries, sectors=None, n_frames: int = 1) -> np.ndarray:
        """dg_sight_device: sight_host() on the GPU, bit for bit (synchronous; touches no slot)."""
        q = _sight_queries(queries)
        out = np.empty(q.size, dtype=np.uint8)
        _check(lib().dg_sight_device(self._h, sectors, n_frames, q.ctypes.data_as(_P), q.size, out.ctypes.data_as(_P)))
        return out

    def sight_mobjs(self, views, eye_height: float, mobj_height, poses=None, sectors=None) -> np.ndarray:
        """dg_sight_mobjs_device: sight_mobjs_host() on the GPU, bit for bit (synchronous; touches no slot)."""
        heights, out = _sight_mobj_args(self._scene, views, mobj_height)
        _check(lib().dg_sight_mobjs_device(self._h, views, poses, sectors, len(views), eye_height, heights.ctypes.data_as(_P), out.ctypes.data_as(_P)))
        return out

    def sight_kernel_ms(self) -> dict:
        """dg_ctx_sight_kernel_ms: GPU time (ms) of the last sight() / sight_mobjs() call's kernels (rows_ms 0: no frame had entries)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().dg_ctx_sight_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"rows_ms": a.value, "sight_ms": b.value}

    def render_state(self, views, states) -> np.ndarray:
        """render() with one game-state snapshot per view (make_view_states)."""
        n = len(views)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_render_views_state(self._h, views, states, n, out.ctypes.data_as(_P)))
        return out

    def submit_depth(self, slot: int, views, n=None, states=None):
        """dg_submit_depth_views: depth + surface-kind frames into the slot, asynchronously (always through the host list path)."""
        _check(lib().dg_submit_depth_views(self._h, slot, views, states, len(views) if n is None else n))

    def render_depth(self, views, states=None, distance: bool = True, kind: bool = True):
        """dg_render_depth_views: synchronous through slot 0; returns (int16 [n,H,W] distance, uint8 [n,H,W] kind)."""
        n = len(views)
        d, k, dp, kp = _depth_planes(n, self.height, self.width, distance, kind)
        _check(lib().dg_render_depth_views(self._h, views, states, n, dp, kp))
        return d, k

    def depth_lists(self, slot: int, frames, distance: bool = True, kind: bool = True):
        """dg_depth_lists: the depth planes of caller-built lists (synchronous); returns (distance, kind)."""
        n = len(frames)
        d, k, dp, kp = _depth_planes(n, self.height, self.width, distance, kind)
        _check(lib().dg_depth_lists(self._h, slot, frames, n, dp, kp))
        return d, k

    def readback_depth(self, slot: int, first: int, count: int, distance: bool = True, kind: bool = True):
        """dg_readback_depth: the planes of frames [first, first + count) of a depth slot; returns (distance, kind)."""
        d, k, dp, kp = _depth_planes(count, self.height, self.width, distance, kind)
        _check(lib().dg_readback_depth(self._h, slot, first, count, dp, kp))
        return d, k

    def submit_labels(self, slot: int, views, n=None, states=None):
        """dg_submit_label_views: object-label frames into the slot, asynchronously (always through the host list path)."""
        _check(lib().dg_submit_label_views(self._h, slot, views, states, len(views) if n is None else n))

    def _label_outputs(self, n: int, id: bool, cls: bool, boxes: bool):
        return _label_outputs(n, self.height, self.width, self._scene.mobj_count(), id, cls, boxes)

    def render_labels(self, views, states=None, id: bool = True, cls: bool = True, boxes: bool = True):
        """dg_render_label_views: synchronous through slot 0; returns (uint16 [n,H,W] id, uint8 [n,H,W] cls, boxes [n, map objects])."""
        out, ptrs = self._label_outputs(len(views), id, cls, boxes)
        _check(lib().dg_render_label_views(self._h, views, states, len(views), *ptrs))
        return out

    def label_lists(self, slot: int, frames, owners, id: bool = True, cls: bool = True, boxes: bool = True):
        """dg_label_lists: the label planes and boxes of caller-built lists with their owner tags (synchronous)."""
        out, ptrs = self._label_outputs(len(frames), id, cls, boxes)
        op, keep = owner_pointers(owners)
        _check(lib().dg_label_lists(self._h, slot, frames, op, len(frames), *ptrs))
        return out

    def readback_labels(self, slot: int, first: int, count: int, id: bool = True, cls: bool = True, boxes: bool = True):
        """dg_readback_labels: the planes and box rows of frames [first, first + count) of a label slot."""
        out, ptrs = self._label_outputs(count, id, cls, boxes)
        _check(lib().dg_readback_labels(self._h, slot, first, count, *ptrs))
        return out

    def label_timing(self, slot: int) -> dict:
        """dg_slot_label_timing: GPU time (ms) of dg_label_tiles and dg_label_boxes of the slot's last submission."""
        t, b = ctypes.c_float(), ctypes.c_float()
        _check(lib().dg_slot_label_timing(self._h, slot, ctypes.byref(t), ctypes.byref(b)))
        return {"tiles_ms": t.value, "boxes_ms": b.value}

    def submit_bundle(self, slot: int, views, what: int, n=None, states=None):
        """dg_submit_bundle_views: the parts `what` names (DG_BUNDLE_*) of the same views into the slot from one list build, asynchronously;
        read them back with readback / frame_checksums / readback_reduced, readback_depth and readback_labels."""
        _check(lib().dg_submit_bundle_views(self._h, slot, views, states, len(views) if n is None else n, what))

    def bundle_lists(self, slot: int, frames, owners, what: int):
        """dg_bundle_lists: a bundle of caller-built lists (owners: their owner tags, needed with DG_BUNDLE_LABELS, else None); waits."""
        op, keep = owner_pointers(owners) if owners is not None else (None, None)
        _check(lib().dg_bundle_lists(self._h, slot, frames, op, len(frames), what))

    def bundle_capacity(self, what: int) -> int:
        """dg_bundle_capacity: the largest n one bundle submission of `what` may carry."""
        return _check(lib().dg_bundle_capacity(self._h, what))

    def bundle_timing(self, slot: int) -> dict:
        """dg_slot_bundle_timing: GPU time (ms) of the colour kernels and of dg_bundle_tiles of the slot's last (bundle) submission."""
        a, b, t = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(lib().dg_slot_bundle_timing(self._h, slot, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t)))
        return {"setup_ms": a.value, "raster_ms": b.value, "tiles_ms": t.value}

    def wait(self, slot: int):
        _check(lib().dg_wait(self._h, slot))

    def prepare(self, slot: int, views):
        _check(lib().dg_prepare_views(self._h, slot, views, len(views)))

    def replay(self, slot: int):
        _check(lib().dg_replay_slot(self._h, slot))

    def readback(self, slot: int, first: int, count: int) -> np.ndarray:
        out = np.empty((count, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_readback(self._h, slot, first, count, out.ctypes.data_as(_P)))
        return out

    def frame_checksums(self, slot: int, first: int, count: int) -> np.ndarray:
        """One uint64 per frame, computed on the GPU (dg_frame_checksums); `frame_checksum` is the host-side twin."""
        out = np.zeros(count, dtype=np.uint64)
        _check(lib().dg_frame_checksums(self._h, slot, first, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def readback_async(self, slot: int, first: int, count: int, host_ptr: int):
        """Queue the D2H copy behind the slot's kernels (own copy stream); complete after wait(slot)."""
        _check(lib().dg_readback_async(self._h, slot, first, count, _P(host_ptr)))

    def readback_reduced(self, slot: int, first: int, count: int, desc) -> np.ndarray:
        """dg_readback_reduced: frames [first, first + count) of the slot, box-downscaled on the GPU; (count, oH, oW, 3) or (count, oH, oW)."""
        d = _reduce_desc(desc)
        out = _reduced_array(count, self.width, self.height, d)
        _check(lib().dg_readback_reduced(self._h, slot, first, count, ctypes.byref(d), out.ctypes.data_as(_P)))
        return out

    def readback_reduced_async(self, slot: int, first: int, count: int, desc, host_ptr: int):
        """dg_readback_reduced_async: the downscale and the D2H copy queued behind the slot's kernels; complete after wait(slot)."""
        _check(lib().dg_readback_reduced_async(self._h, slot, first, count, ctypes.byref(_reduce_desc(desc)), _P(host_ptr)))

    def reduce_device(self, src_ptr: int, width: int, height: int, n_frames: int, desc, dst_ptr: int):
        """dg_reduce_device: n_frames RGB24 frames at device address src_ptr downscaled into device address dst_ptr (synchronous; a slot's
        framebuffer_ptr or a tensor's data_ptr(), any alignment).  Touches no slot."""
        _check(lib().dg_reduce_device(self._h, _P(src_ptr), width, height, n_frames, ctypes.byref(_reduce_desc(desc)), _P(dst_ptr)))

    def readback_planes_reduced(self, slot: int, first: int, count: int, desc, distance: bool = True, kind: bool = True, id: bool = True,
                                cls: bool = True, boxes: bool = True) -> dict:
        """dg_readback_planes_reduced: the planes asked for of frames [first, first + count) of a depth, label or bundle slot, reduced on the
        GPU under desc (a DgPlaneReduceDesc, or (fx, fy[, rule])), and the full-size boxes; {name: array} for what was asked for."""
        d = _plane_reduce_desc(desc)
        ow, oh = plane_reduced_size(self.width, self.height, d)
        out = {k: np.empty((count, oh, ow), dtype=PLANE_DTYPES[k]) for k, want in zip(PLANE_NAMES, (distance, kind, id, cls)) if want}
        if boxes:
            out["boxes"] = np.empty((count, self._scene.mobj_count()), dtype=LABEL_BOX_DTYPE)
        ptrs = [out[k].ctypes.data_as(_P) if k in out else None for k in PLANE_NAMES + ("boxes",)]
        _check(lib().dg_readback_planes_reduced(self._h, slot, first, count, ctypes.byref(d), *ptrs))
        return out

    def readback_planes_reduced_async(self, slot: int, first: int, count: int, desc, distance: int = 0, kind: int = 0, id: int = 0, cls: int = 0,
                                      boxes: int = 0):
        """dg_readback_planes_reduced_async: the reduction and the copies queued behind the slot's kernels; each output is a host address
        (0: not asked for) and is complete after wait(slot)."""
        ptrs = [_P(p) if p else None for p in (distance, kind, id, cls, boxes)]
        _check(lib().dg_readback_planes_reduced_async(self._h, slot, first, count, ctypes.byref(_plane_reduce_desc(desc)), *ptrs))

    def reduce_planes_device(self, width: int, height: int, n_frames: int, desc, src: dict, dst: dict):
        """dg_reduce_planes_device: n_frames planes at the device addresses src[name] reduced into the device addresses dst[name]
        (names of PLANE_NAMES; synchronous; planes of a finished slot's framebuffer_ptr or tensors' data_ptr()).  Touches no slot."""
        ptr = lambda d: [_P(d[k]) if d.get(k) else None for k in PLANE_NAMES]
        _check(lib().dg_reduce_planes_device(self._h, width, height, n_frames, ctypes.byref(_plane_reduce_desc(desc)), *ptr(src), *ptr(dst)))

    def observe_device(self, src_ptr: int, width: int, height: int, n_frames: int, desc: DgObsDesc, dst_ptr: int, strides):
        """dg_observe_device: n_frames sources at device address src_ptr observed under desc into the (N, C, H, W) destination at device
        address dst_ptr whose strides, in elements, are `strides` (synchronous; touches no slot)."""
        _check(lib().dg_observe_device(self._h, _P(src_ptr), width, height, n_frames, ctypes.byref(desc), _P(dst_ptr), (ctypes.c_int64 * 4)(*[int(v) for v in strides])))

    def observe_into(self, src_ptr: int, width: int, height: int, n_frames: int, desc: DgObsDesc, tensor):
        """observe_device into a tensor, or a view of one, of shape (n_frames, C, oH, oW) and the descriptor's dtype: anything with
        .shape, .stride() in elements, .data_ptr() and a dtype whose name ends in uint8 / float16 / bfloat16 / float32.  ValueError when
        shape or dtype are not what observed_size says."""
        c, oh, ow, _ = observed_size(width, height, desc)
        if tuple(int(v) for v in tensor.shape) != (n_frames, c, oh, ow):
            raise ValueError(f"observe_into: the tensor's shape {tuple(tensor.shape)} is not {(n_frames, c, oh, ow)}")
        if str(tensor.dtype).split(".")[-1] != OBS_DTYPE_NAMES[desc.dtype]:
            raise ValueError(f"observe_into: the tensor's dtype {tensor.dtype} is not {OBS_DTYPE_NAMES[desc.dtype]}")
        self.observe_device(src_ptr, width, height, n_frames, desc, tensor.data_ptr(), tensor.stride())

    def observe_kernel_ms(self) -> float:
        """dg_ctx_observe_kernel_ms: GPU time of the last observe_device call's kernel."""
        ms = ctypes.c_float()
        _check(lib().dg_ctx_observe_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def overlay_device(self, frames_ptr: int, width: int, height: int, items_per_frame):
        """dg_overlay_device: the screen pictures items_per_frame (screen_pictures: one list per frame) drawn on the RGB24 frames at
        device address frames_ptr (synchronous; touches no slot)."""
        items, first = screen_pictures(items_per_frame)
        _check(lib().dg_overlay_device(self._h, _P(frames_ptr), width, height, len(items_per_frame), items.ctypes.data_as(_P), first.ctypes.data_as(_P)))

    def slot_overlay(self, slot: int, first_frame: int, items_per_frame):
        """dg_slot_overlay: the screen pictures items_per_frame drawn on the colour frames first_frame .. of the slot's last submission,
        one list per frame, once the submission is final."""
        items, first = screen_pictures(items_per_frame)
        _check(lib().dg_slot_overlay(self._h, slot, first_frame, len(items_per_frame), items.ctypes.data_as(_P), first.ctypes.data_as(_P)))

    def overlay_kernel_ms(self) -> float:
        """dg_ctx_overlay_kernel_ms: GPU time of the last overlay_device / slot_overlay call's kernel."""
        ms = ctypes.c_float()
        _check(lib().dg_ctx_overlay_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def plane_reduce_kernel_ms(self) -> float:
        """dg_ctx_plane_reduce_kernel_ms: GPU time of the last reduce_planes_device call's kernel."""
        ms = ctypes.c_float()
        _check(lib().dg_ctx_plane_reduce_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def reduce_kernel_ms(self) -> float:
        """dg_ctx_reduce_kernel_ms: GPU time of the last reduce_device call's kernel."""
        ms = ctypes.c_float()
        _check(lib().dg_ctx_reduce_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def fallbacks(self) -> dict:
        a, f = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().dg_ctx_fallbacks(self._h, ctypes.byref(a)))
        _check(lib().dg_ctx_redone_frames(self._h, ctypes.byref(f)))
        return {"front_end": a.value, "redone_frames": f.value}

    def readback_into(self, slot: int, first: int, count: int, host_ptr: int):
        _check(lib().dg_readback(self._h, slot, first, count, _P(host_ptr)))

    def framebuffer_ptr(self, slot: int) -> int:
        p = _P()
        _check(lib().dg_slot_framebuffer(self._h, slot, ctypes.byref(p)))
        return p.value

    def draw_lists(self, slot: int, frames) -> np.ndarray:
        n = len(frames)
        out = np.empty((n, self.height, self.width, 3), dtype=np.uint8)
        _check(lib().dg_draw_lists(self._h, slot, frames, n, out.ctypes.data_as(_P)))
        return out

    def locate_walks(self, walks):
        """dg_ctx_locate_walks: the floor heights of all these walks in one pass on the GPU (synchronous; located walks are skipped)."""
        arr = (_P * max(1, len(walks)))(*[w._h for w in walks])
        _check(lib().dg_ctx_locate_walks(self._h, arr, len(walks)))

    def timing(self, slot: int) -> dict:
        t = DgTiming()
        _check(lib().dg_slot_timing(self._h, slot, ctypes.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def close(self):
        if self._h:
            lib().dg_destroy(self._h)
            self._h = None


def frame_checksum(rgb24) -> int:
    """dg_frame_checksums' formula on the host, for one frame given as bytes / uint8 array of length 3*W*H (a byte count that is not a
    multiple of 4 ends in a zero-extended partial dword)."""
    raw = bytes(rgb24) if not isinstance(rgb24, np.ndarray) else np.ascontiguousarray(rgb24).reshape(-1).tobytes()
    raw += b"\0" * (-len(raw) % 4)
    d = np.frombuffer(raw, dtype="<u4")
    with np.errstate(over="ignore"):
        i = np.arange(d.size, dtype=np.uint64)
        m = (d.astype(np.uint64) ^ (i * np.uint64(0x9E3779B97F4A7C15))) * np.uint64(0xBF58476D1CE4E5B9)
        return int((m ^ (m >> np.uint64(32))).sum(dtype=np.uint64))


def declared_symbols() -> list[str]:
    """Function names declared in include/doomgpu.h (for the export check)."""
    import re
    txt = open(INCLUDE).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dg_[a-z_0-9]+)\s*\(", txt)))
