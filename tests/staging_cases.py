"""Hand-built lists aimed at the staging limit of dg_depth_tiles / dg_label_tiles / dg_bundle_tiles (16 spans per column in LDS; span 16 and later are
resolved from the list slab inside the row loop) and at the run and piece boundaries of dg_label_boxes.  Beside tests/depth_cases.py, in
the same list-dict form; shared by tests/test_staging_cases_host.py (host entries == the numpy models) and tests/test_plane_shapes_gpu.py.
Both builders work at any W x H >= 1 x 1.

  ladder      adjacent columns carry 0, 1, 7, 8, 9, 15, 16, 17, 24 and 33 spans, the pattern shifted so that columns 63 | 64 carry 16 | 17.
              Draw command s ("slot") has a span on exactly the columns that carry more than s spans, so a span's index in its column IS its
              slot; the slots cycle flat, opaque wall, sky, holey wall, so that slot 16 (the first one past the staging) is a flat, 18 a sky
              plane, 17 and 19 walls.  A plane slot is cut into one visplane per run of adjacent columns that take part.
  box_edges   map-object columns (opaque wall records with hand-given map-object owners) on a floor: see the function.
"""
import numpy as np

from test_edge_kats import wall

LADDER = [0, 1, 7, 8, 9, 15, 16, 17, 24, 33]
SLOTS = max(LADDER)
FLAT, OPAQUE, SKY, HOLEY = range(4)
SYNTH = {"opaque": ["BRICK1", "STONE2", "METAL2", "PANEL2"], "holey": ["HOLEY1", "GRATE1", "COMBO2"], "flat": ["FLOOR1", "CEIL2", "FLOOR3", "NUKAGE1"]}
HAND = {"opaque": ["WALLA"], "holey": ["MASKED", "TWOP"], "flat": ["FLOORA", "CEILA", "NUKAGE1"]}      # tests/test_hand_wad.py
LADDER_VIEW = (310.0, -95.5, 1.9, 8.0)
BOX_VIEW = (0.0, 0.0, -2.1, 16.0)


def bundle_batch_for(dg, W, H, n, what=7):
    """The smallest max_batch whose framebuffer slab holds a bundle of n frames with the parts `what` (default: all three)."""
    return max(n, -(-dg.bundle_layout(W, H, n, what)["total"] // (3 * W * H)))


def ladder_count(x):
    return LADDER[(x + 3) % len(LADDER)]


def slot_kind(s):
    return s % 4


def slot_rows(s, x, H):
    """Rows of slot s on column x: a third of the frame (three rows at least, so that a flat column is not skipped where H allows),
    placed so that neighbouring slots and columns overlap only in part."""
    hgt = min(H, max(3, H // 3))
    top = (11 * s + 3 * x) % (H - hgt + 1)
    return top, min(H - 1, top + hgt - 1 + (s + x) % 3)


def ladder(W, H, names=SYNTH):
    columns, renders, planes, order, slots = [], [], [], [], []
    for s in range(SLOTS):
        xs = [x for x in range(W) if ladder_count(x) > s]
        if not xs:
            continue
        k = slot_kind(s)
        if k in (OPAQUE, HOLEY):
            tex = names["holey" if k == HOLEY else "opaque"][(s // 4) % len(names["holey" if k == HOLEY else "opaque"])]
            cols = []
            for x in xs:
                ct, cb = slot_rows(s, x, H)
                cols.append((x, ct, cb, cb + 2, ct - 1))
            order.append((0, len(renders)))
            slots.append(s)
            renders.append(wall(tex, 255 - 5 * s, (50.0 + 3 * s, -10.0 - s, 64.0 + 2 * s, 12.0), 0, W - 1, -41.0, 87.0, cols, columns, offset_x=7 * s, offset_y=-3 * s))
        else:
            runs, run = [], [xs[0]]
            for x in xs[1:]:
                if x == run[-1] + 1:
                    run.append(x)
                else:
                    runs.append(run)
                    run = [x]
            runs.append(run)
            for run in runs:
                order.append((1, len(planes)))
                slots.append(s)
                flat = "F_SKY1" if k == SKY else names["flat"][(s // 4) % len(names["flat"])]
                planes.append({"flat": flat, "height": 128 if k == SKY else (-16 + 24 * ((s // 4) % 3)), "light_level": 255 if k == SKY else 120 + 4 * s,
                               "left": run[0], "right": run[-1], "tb": [slot_rows(s, x, H) for x in run]})
    return {"renders": renders, "columns": columns, "visplanes": planes, "order": order, "slots": slots}       # slots: order index -> slot


def ladder_cover(W, H, lists):
    """-> bool [order index][H][W]: the rows each draw command's spans cover (clamped to the frame)."""
    cover = np.zeros((len(lists["order"]), H, W), dtype=bool)
    for t, (kind, idx) in enumerate(lists["order"]):
        if kind == 0:
            r = lists["renders"][idx]
            for (x, ct, cb, _b, _t) in lists["columns"][r["first_column"]:r["first_column"] + r["n_columns"]]:
                cover[t, max(0, ct):min(H - 1, cb) + 1, x] = True
        else:
            p = lists["visplanes"][idx]
            for i, x in enumerate(range(p["left"], p["right"] + 1)):
                cover[t, max(0, p["tb"][i][0]):min(H - 1, p["tb"][i][1]) + 1, x] = True
    return cover


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------------

def box_edges(W, H, n_mobjs, n_segs=1000):
    """-> (lists, owner tags, {role: map object}).  On a floor plane over the whole frame, in draw order:
      everywhere   one row across every column (visible in every 64-column strip), drawn first so that the others cut it
      corners      object 0: four one-pixel runs at (0, H/2), (W/2, 0), (W-1, H/3), (W/3, H-1) — its box is the whole frame
      single       object n_mobjs - 1: one pixel
      upto31/from32, upto127/from128   in one column each, a run that ends on row 31 (127) and another object's that starts on row 32 (128):
                   the last row of one 32-row piece (128-row band) and the first of the next
      split        two runs in one column with `between` (three rows of another object) in the middle
      hidden       drawn, then covered completely by a wall record (class wall): its box is -1
    """
    assert n_mobjs >= 12
    role = {"corners": 0, "single": n_mobjs - 1, "everywhere": 1, "upto31": 2, "from32": 3, "upto127": 4, "from128": 5, "split": 6, "between": 7, "hidden": 8}
    X = lambda v: max(0, min(W - 1, v))
    Y = lambda v: max(0, min(H - 1, v))
    columns, renders, owners = [], [], []

    def record(who, cols, tex="BRICK1", wall_owner=None):
        cols = [(X(x), Y(t), Y(b), Y(b) + 1, Y(t) - 1) for (x, t, b) in cols if t <= b and t < H]
        renders.append(wall(tex, 200, (70.0 + len(renders), -20.0, 90.0 + len(renders), 25.0), 0, W - 1, -41.0, 87.0, cols, columns, offset_x=3 * len(renders)))
        owners.append((1 << 16) | wall_owner if wall_owner is not None else (2 << 16) | role[who])

    row = Y(H - 3)
    record("everywhere", [(x, row, row) for x in range(W)])
    record("corners", [(0, H // 2, H // 2), (W // 2, 0, 0), (W - 1, H // 3, H // 3), (W // 3, H - 1, H - 1)])
    record("single", [(W // 2 + 1, H // 2 + 1, H // 2 + 1)])
    x1, x2, x3 = (5 * W) // 8, W // 4, (7 * W) // 8
    record("upto31", [(x1, 24, 31)])
    record("from32", [(x1, 32, 36)])
    record("upto127", [(x1 + 2, 119, 127)])
    record("from128", [(x1 + 2, 128, 140)])
    record("split", [(x2, 3, 19)], tex="STONE2")
    record("between", [(x2, 9, 11)])
    record("hidden", [(x, 4, 9) for x in range(x3, x3 + 3)], tex="METAL2")
    record(None, [(x, 2, 12) for x in range(x3 - 1, x3 + 4)], tex="PANEL2", wall_owner=37 % n_segs)
    planes = [{"flat": "FLOOR1", "height": -16, "light_level": 160, "left": 0, "right": W - 1, "tb": [(0, H - 1)] * W}]
    lists = {"renders": renders, "columns": columns, "visplanes": planes, "order": [(1, 0)] + [(0, i) for i in range(len(renders))]}
    return lists, np.array(owners, dtype=np.uint32), role
