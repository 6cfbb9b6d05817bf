"""Hand-built draw lists for the depth / surface-kind frame: the corners of tests/test_edge_kats.py restated for depth, in the list-dict
form np_mappers.draw_lists replays (and test_edge_kats.to_dg_lists turns into dg_frame_lists).  Shared by test_depth_host.py (host entry
== the np_depth model) and test_depth_gpu.py (GPU == host entry).  Every case is a function of the frame size; at 64x40 CFY = 20, so that
row 20 has vy == 0.
"""
from test_dense_columns import many_records, seventy_spans
from test_edge_kats import wall


def horizon(W, H):
    """Floor / ceiling planes across the vy == 0 row (H even) with wz < 0, wz > 0 and wz == 0 (gwz / 0 = -inf, +inf, NaN -> -32768, 32767,
    0), the `bottom - top <= 1` skip next to a drawn column, and a sky plane laid over a wall."""
    mid = H // 2
    w3 = max(1, W // 3)
    columns = []
    renders = [wall("BRICK1", 160, (100.0, -30.0, 180.0, 50.0), 0, W - 1, -41.0, 87.0, [(x, 0, min(H - 1, 6), 30, -4) for x in range(W)], columns)]
    planes = [
        {"flat": "FLOOR1", "height": 0, "light_level": 300, "left": 0, "right": w3 - 1, "tb": [(max(0, mid - 3 - x % 3), H - 1) for x in range(w3)]},         # wz = -41
        {"flat": "CEIL2", "height": 128, "light_level": -20, "left": w3, "right": min(W - 1, 2 * w3 - 1), "tb": [(0, min(H - 1, mid + x % 2)) for x in range(w3, min(W, 2 * w3))]},   # wz = 87
        {"flat": "FLOOR0", "height": 41, "light_level": 200, "left": min(W - 1, 2 * w3), "right": W - 1, "tb": [(-5, 2 * H)] * (W - min(W - 1, 2 * w3))},     # wz = 0: NaN on the horizon row
        {"flat": "NUKAGE1", "height": -24, "light_level": 144, "left": 0, "right": W - 1, "tb": [(H - 4, H - 4 + x % 4) for x in range(W)]},                  # bottom - top = 0, 1 (skipped), 2, 3
        {"flat": "F_SKY1", "height": 128, "light_level": 255, "left": 0, "right": W - 1, "tb": [(0, x % 4) for x in range(W)]},                             # sky over the wall's first rows
    ]
    return {"renders": renders, "columns": columns, "visplanes": planes, "order": [(0, 0)] + [(1, i) for i in range(len(planes))]}


def wall_corners(W, H):
    """bottom_y == top_y (the NaN row: ownership follows the texel the reference picks — HOLEY1 has holes), uz0 == 0, columns at
    x >= W and x < 0, saturated extents, a zero-length line."""
    columns = []
    m = H // 2
    renders = [
        wall("BRICK1", 160, (100.0, -30.0, 180.0, 50.0), 0, W - 1, -41.0, 87.0, [(x, 1, H - 2, H - 2 + x // 8, 1 - x // 16) for x in range(W)], columns),
        wall("HOLEY1", 255, (60.0, 10.0, 90.0, -20.0), 0, W - 1, -10.0, 62.0, [(x, max(0, m - 2), min(H - 1, m + 2), m, m) for x in range(0, W, 2)], columns, offset_x=17, offset_y=-7),
        wall("WIDE2", 96, (0.0, -12.0, 40.0, 8.0), 0, 40, -41.0, 15.0, [(x, min(H - 1, m + 3), H - 1, H - 1, m + 3) for x in range(0, min(W, 41))], columns, offset_x=-300, start_offset=13.7),
        wall("PANEL2", 224, (5.0, 1.0, 5.25, -1.0), W // 2, W - 1, -2000.0, 2000.0, [(x, 0, H - 1, 32767, -32768) for x in range(W // 2, W, 3)], columns, offset_y=30000),
        wall("BRICK3", 128, (50.0, 5.0, 70.0, -5.0), W - 4, W + 6, -41.0, 40.0, [(x, 0, min(H - 1, 4), 12, 0) for x in (-3, W - 4, W - 1, W, W + 6, 32767, -32768)], columns),
        wall("BRICK2", 192, (64.0, 0.0, 64.0, 0.0), 2, 2, -41.0, 87.0, [(min(2, W - 1), 0, H - 1, H - 1, 0)], columns),
    ]
    return {"renders": renders, "columns": columns, "visplanes": [], "order": [(0, i) for i in range(len(renders))]}


def masked_over_floor(W, H):
    """A floor plane, then a masked texture (GRATE1) drawn in one- and two-row columns: wherever every texel of such a column is
    transparent the pixel keeps the floor's kind and distance; then HOLEY1 and an opaque wall over part of it, then a ceiling again."""
    columns = []
    m = H // 2
    planes = [{"flat": "FLOOR3", "height": -8, "light_level": 176, "left": 0, "right": W - 1, "tb": [(0, H - 1)] * W},
              {"flat": "CEIL0", "height": 96, "light_level": 112, "left": W // 3, "right": W // 2, "tb": [(1, min(H - 1, 4))] * (W // 2 - W // 3 + 1)}]
    renders = [
        wall("GRATE1", 255, (40.0, -20.0, 44.0, 20.0), 0, W - 1, -41.0, 87.0, [(x, m, min(H - 1, m + x % 2), 45, -6) for x in range(W)], columns, offset_y=-200),
        wall("HOLEY1", 208, (80.0, -40.0, 120.0, 40.0), 0, W - 1, -41.0, 87.0, [(x, 0, max(0, m - 2), 36, 4) for x in range(W)], columns, offset_x=5),
        wall("STONE2", 96, (90.0, 0.0, 91.0, 30.0), W // 2, W // 2 + 4, -41.0, 87.0, [(x, 0, H - 1, H - 1, 0) for x in range(W // 2, min(W, W // 2 + 5))], columns),
    ]
    return {"renders": renders, "columns": columns, "visplanes": planes, "order": [(1, 0), (0, 0), (0, 1), (0, 2), (1, 1)]}


def dense_strip(W, H):
    """24 records on every column: more spans per column than dg_depth_tiles stages in LDS (16), on every strip of the frame."""
    return many_records(W, H)


def seventy(W, H):
    """test_dense_columns' 70-span column (needs W >= 24)."""
    return seventy_spans(W, H)


VIEWS = {"horizon": (1000.3, -740.8, 0.7, 0.0), "wall_corners": (0.0, 0.0, -2.1, 16.0), "masked_over_floor": (-512.0, 2048.5, 3.9, -24.0),
         "dense_strip": (0.0, 0.0, -2.1, 16.0), "seventy": (-100.0, 300.0, 0.4, 0.0)}
BUILDERS = {"horizon": horizon, "wall_corners": wall_corners, "masked_over_floor": masked_over_floor, "dense_strip": dense_strip, "seventy": seventy}


def cases(W, H):
    """-> [(name, view (x, y, angle, floor), lists)] at W x H; the 70-span column only where the frame has its columns 20..23."""
    return [(n, VIEWS[n], BUILDERS[n](W, H)) for n in BUILDERS if n != "seventy" or W >= 24]
