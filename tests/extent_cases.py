"""What the CPU and GPU tiers of the band kernels' extents share (tests/test_extents_host.py, tests/test_extents_gpu.py,
tests/extents/torch_cases.py): the launch plan of launch_reduce, launch_plane_reduce and launch_observe restated in Python, the classes
of launch the suite has to reach, the shape table that reaches them, and the frame counts and sizes of the cases past one launch and
past 2^32.

A band kernel (dg_reduce<>, dg_observe_rgb<> : family "colour"; dg_plane_nearest<>, dg_observe_distance_nearest<> : family "column")
splits a row of oW output pixels into runs of px_per_wg(fx); run r starts at output pixel ox0 = r * px_per_wg, holds
np = min(px_per_wg, oW - ox0) of them, and its first source unit (a byte of an RGB row, a column of a plane) is first = unit * ox0 with
unit = 3 fx bytes or fx columns.  The 16-byte form of the kernel (3 W % 16 == 0 or W % 8 == 0, and a 16-byte aligned base) starts
reading at first rounded down to a piece, off0 = first % 16 bytes or first % 8 columns in front of it; the any-width form has off0 = 0.
The point kernels (dg_plane_point, dg_observe_distance_point: family "point") take blocks of 256 output pixels, a lane each."""
import numpy as np

import np_reduce as npr

LANES = 256
REDUCE_SPAN = LANES * 16                # bytes of an RGB row one workgroup's lanes read as 16-byte pieces
PLANE_REDUCE_SPAN = LANES * 8           # columns of a distance plane, likewise
FAMILIES = ("colour", "column", "point")
MAX_EXTENT = 16384
CHUNK = 65535                           # frames per launch: the grid's z (y for dg_seen_lines) extent


def reduce_px_per_wg(fx):
    return (REDUCE_SPAN - 15) // (3 * fx)


def plane_reduce_px_per_wg(fx):
    return (PLANE_REDUCE_SPAN - 7) // fx


def launch_plan(family, W, fx, base_off=0):
    """What the launcher and the kernel do with a row of W source pixels under box width fx, the source base_off BYTES behind a 16-byte
    boundary: {"pieces": the 16-byte form, "runs": [(np, off0), ...], "short_box": the row's last box has fewer than fx columns}.
    For "point" a run is a block of 256 lanes, np its live lanes, and pieces is False."""
    oW = -(-W // fx)
    if family == "point":
        per, unit, piece, pieces = LANES, 0, 1, False
    elif family == "colour":
        per, unit, piece, pieces = reduce_px_per_wg(fx), 3 * fx, 16, (3 * W) % 16 == 0 and base_off % 16 == 0
    else:
        assert family == "column"
        per, unit, piece, pieces = plane_reduce_px_per_wg(fx), fx, 8, W % 8 == 0 and base_off % 16 == 0
    runs = []
    for ox0 in range(0, oW, per):
        runs.append((min(per, oW - ox0), (unit * ox0) % piece if pieces else 0))
    return {"pieces": pieces, "per": per, "runs": runs, "short_box": W % fx != 0}


def count_class(n):
    return "1" if n == 1 else "2" if n == 2 else ">=3"


def launch_classes(family, W, H, fx, fy, base_off=0):
    """The classes one case reaches: tuples that start with the family and, for the band kernels, the form ("16-byte" / "any-width")."""
    p = launch_plan(family, W, fx, base_off)
    runs, n = p["runs"], len(p["runs"])
    if family == "point":
        c = {("point", "blocks", count_class(n))}
        if n >= 2 and runs[-1][0] == 1:
            c.add(("point", "last block of one lane"))
        return c
    form = "16-byte" if p["pieces"] else "any-width"
    c = {(family, form, "runs", count_class(n))}
    if n >= 2:
        last = runs[-1][0]
        c.add((family, form, "last run", "full" if last == p["per"] else "one pixel" if last == 1 else "in between"))
        c.add((family, form, "last band", "short" if H % fy else "full"))
        if p["short_box"]:
            c.add((family, form, "short last box in a later run"))
        if p["pieces"]:
            c |= {(family, form, "off0 in a later run", "!= 0" if off0 else "== 0") for _, off0 in runs[1:]}
        else:
            piece_width = (3 * W) % 16 == 0 if family == "colour" else W % 8 == 0
            c.add((family, form, "reached by", "base" if piece_width else "width"))
    if W == MAX_EXTENT:
        c.add((family, form, "W = 16384"))
    if H == MAX_EXTENT and fy == 1:
        c.add((family, form, "H = 16384 with fy = 1"))
    return c


def item_map_classes(W, fx):
    """obs_item's two maps at the runs an RGB observation has (16-byte or not): planar (strides[3] == 1) and interleaved both run at
    every case, so a case reaches ("item maps", "short last run") and ("item maps", "full run other than the first") by its runs alone."""
    p = launch_plan("colour", W, fx)
    c = set()
    if len(p["runs"]) >= 2 and p["runs"][-1][0] < p["per"]:
        c.add(("item maps", "short last run"))
    if any(n == p["per"] for n, _ in p["runs"][1:]):
        c.add(("item maps", "full run other than the first"))
    return c


def required_classes():
    need = set()
    for family in ("colour", "column"):
        for form in ("16-byte", "any-width"):
            need |= {(family, form, "runs", k) for k in ("1", "2", ">=3")}
            need |= {(family, form, "last run", k) for k in ("full", "one pixel", "in between")}
            need |= {(family, form, "last band", k) for k in ("full", "short")}
            need.add((family, form, "short last box in a later run"))
            need.add((family, form, "W = 16384"))
        need |= {(family, "16-byte", "off0 in a later run", k) for k in ("!= 0", "== 0")}
        need |= {(family, "any-width", "reached by", k) for k in ("width", "base")}
        need.add((family, "any-width", "H = 16384 with fy = 1"))            # (3 x 16384: three columns are no 16-byte row)
    need |= {("point", "blocks", k) for k in ("1", "2", ">=3")}
    need.add(("point", "last block of one lane"))
    need |= {("item maps", "short last run"), ("item maps", "full run other than the first")}
    return need


# ---- the shape table -------------------------------------------------------------------------------------------------------------------
# (W, H, unaligned): H None = 5 rows, 17 under fy = 16 (a full band and a last band of one or two rows at every fy of np_reduce.FACTORS);
# unaligned = the source sits 1 byte (colour) or 2 bytes (distance) behind a 16-byte boundary.  Every shape runs under every box size of
# np_reduce.FACTORS.  What each width is here for, with R = reduce_px_per_wg, P = plane_reduce_px_per_wg:
SHAPES = [
    (1360, None, False),     # R(1) = 1360: one full colour run; fx 3 / 7: a second colour run of ONE pixel whose box is short (16-byte form)
    (1361, None, False),     # any-width colour: fx 1 a second run of one pixel
    (1376, None, False),     # 16-byte colour: fx 16: 85 + 1 pixels; off0 == 0 and != 0 in second runs
    (2041, None, False),     # P(1) = 2041: one full column run, any-width; two colour runs
    (2042, None, False),     # any-width columns: fx 1 a second run of one pixel; short boxes in second runs
    (2048, None, False),     # 16-byte columns: fx 16: 127 + 1 pixels; fx 1: off0 = 1 in the second run
    (2720, None, False),     # 16-byte colour: fx 1 two FULL runs; fx 3: off0 = 13, fx 7: off0 = 10; 16-byte columns: fx 7: off0 = 5
    (2720, None, True),      # the same rows by the any-width kernels: reached by the base at a 16-byte width, full last colour run
    (4080, None, False),     # 16-byte: three full colour runs under fx 1; two full column runs under fx 2, 3, 4
    (4080, None, True),      # any-width columns with a full last run
    (4088, None, False),     # any-width colour (3 W % 16 = 8), 16-byte columns: >= 3 runs in both
    (4112, None, False),     # 16-byte both: >= 3 runs, short boxes in third runs
    (4113, None, False),     # any-width both: >= 3 runs; fx 1: a third column run of 31, a fourth colour run of 33
    (513, None, False),      # point kernels: 513 = 2 * 256 + 1 output pixels under fx 1 (a third block of one lane), 257 under fx 2
    (16384, 2, False),       # the contract's widest row: 13 colour runs, 9 column runs, 64 point blocks under fx 1
    (16384, 2, True),        # the same rows by the any-width kernels
    (3, 16384, False),       # the contract's tallest frame: 16384 bands under fy = 1
]
FRAMES = 2                   # frames per case: the second frame's offset is no multiple of 16 at the odd widths


def height_of(H, fy):
    return H if H is not None else 17 if fy == 16 else 5


def cases():
    """Every (W, H, fx, fy, unaligned) of the table."""
    return [(W, height_of(H, fy), fx, fy, un) for (W, H, un) in SHAPES for (fx, fy) in npr.FACTORS]


def shape_id(shape):
    W, H, un = shape
    return f"{W}x{'band' if H is None else H}{'_off' if un else ''}"


def reached():
    got = set()
    for (W, H, fx, fy, un) in cases():
        got |= launch_classes("colour", W, H, fx, fy, 1 if un else 0)
        got |= launch_classes("column", W, H, fx, fy, 2 if un else 0)
        got |= launch_classes("point", W, H, fx, fy)
        got |= item_map_classes(W, fx)
    return got


def colour_frames(W, H):
    """One frame of every content of np_reduce.CONTENTS: (5, H, W, 3) uint8."""
    return np.concatenate([npr.content(kind, 1, W, H, seed=i) for i, kind in enumerate(npr.CONTENTS)])


def plane_sources(W, H, fx, fy):
    """One frame of every distance content of np_plane_reduce.CONTENTS with tracer planes that differ per frame (frame f is
    np_plane_reduce.tracer_planes shifted by 7919 f): {name: (4, H, W)}.  An output then names the frame and the source pixel taken,
    also where W * H > 65 536."""
    import np_plane_reduce as npp
    n = len(npp.CONTENTS)
    y, x = np.mgrid[0:H, 0:W]
    ids = np.stack([((y * W + x + 7919 * f) & 0xFFFF).astype(np.uint16) for f in range(n)])
    assert np.array_equal(ids[0], npp.tracer_planes(1, W, H)["id"][0])
    planes = {"kind": ((ids >> 3) & 3).astype(np.uint8), "id": ids, "cls": (ids & 7).astype(np.uint8)}
    planes["distance"] = np.concatenate([npp.distance_content(kind, 1, W, H, fx, fy, seed=i) for i, kind in enumerate(npp.CONTENTS)])
    return planes


# ---- past the first launch ---------------------------------------------------------------------------------------------------------------
FRAME_COUNTS = (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)       # 65535 (one launch: the control), 65536, 131070, 131071
# entry point -> ((W, H) of the 16-byte kernel, (W, H) of the any-width kernel)
CHUNK_SHAPES = {"reduce": ((16, 2), (3, 2)), "planes": ((8, 2), (3, 2)), "observe_rgb": ((16, 2), (3, 2)), "observe_distance": ((8, 2), (3, 2)),
                "seen": ((16, 1), (3, 2))}


def random_frames(n, H, W, seed):
    return np.random.default_rng([seed, W, H, n]).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def random_distance(n, H, W, seed):
    return np.random.default_rng([seed, W, H, n]).integers(-32768, 32768, size=(n, H, W), dtype=np.int64).astype(np.int16)


def random_labels(n, H, W, n_segs, seed):
    """id (n, H, W) uint16 over [0, n_segs + 8) and cls (n, H, W) uint8 over 0..4 (1 = wall), random per pixel."""
    rng = np.random.default_rng([seed, W, H, n])
    return rng.integers(0, n_segs + 8, size=(n, H, W), dtype=np.uint16), rng.integers(0, 5, size=(n, H, W), dtype=np.uint8)


def seen_rows(ex, ids, cls):
    """np_explored.Explored.seen for many small frames at once: (n, words) uint32."""
    n = ids.shape[0]
    f, y, x = np.nonzero((cls == 1) & (ids < len(ex.seg_line)))
    line = np.asarray(ex.seg_line, dtype=np.int64)[ids[f, y, x].astype(np.int64)]
    out = np.zeros((n, ex.words), dtype=np.uint32)
    np.bitwise_or.at(out, (f, line >> 5), (np.uint32(1) << (line & 31).astype(np.uint32)))
    return out


# ---- past 2^32 -----------------------------------------------------------------------------------------------------------------------------
TWO32 = 1 << 32
K_BASE = 3                              # distinct base frames a source past 2^32 is tiled from (odd)
# source cases: entry -> (W, H, bytes per pixel of the plane that passes 2^32): 259 rows = 16 bands of 16 and one of 3; 2^32 is no multiple
# of the frame's bytes
BIG_SOURCES = {
    "reduce": (1360, 259, 3),           # 1 056 720 B per frame, 16-byte kernel
    "planes": (2048, 259, 2),           # 1 060 864 B of distance (and of id) per frame, 16-byte kernel
    "observe_rgb": (1361, 259, 3),      # any-width
    "observe_distance": (2042, 259, 2),
    "seen": (2048, 259, 2),             # the id plane; cls is half of it
}


def first_frame_behind(frame_bytes):
    """The first frame whose byte offset is at or past 2^32, and where a 32-bit offset would land instead."""
    f = -(-TWO32 // frame_bytes)
    return f, (f * frame_bytes) % TWO32


def big_frames(frame_bytes):
    """Frames of a source past 2^32: a multiple of K_BASE with at least two frames behind the boundary (about 4 060 frames of 1 MB)."""
    f, _ = first_frame_behind(frame_bytes)
    return K_BASE * -(-(f + 2) // K_BASE)


def wrapped_bytes_differ(base, f, wrapped, length=4096):
    """base (K, bytes-per-frame) uint8: the K base frames a tiled source is made of.  True when the first `length` bytes of frame f differ
    from the bytes at byte offset `wrapped` of the tiled source: a condition on the inputs, so that a 32-bit frame offset cannot pass."""
    K, fb = base.shape
    own = base[f % K, :length]
    at = (wrapped + np.arange(length)) % (K * fb)
    return not np.array_equal(own, base.reshape(-1)[at])
