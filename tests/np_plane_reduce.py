"""Numpy restatement of the reduced depth and label planes (include/doomgpu.h: dg_plane_reduce_desc), written from the contract's text:
oW = ceil(W / fx), oH = ceil(H / fy); box (ox, oy) covers source columns [ox*fx, min(W, ox*fx + fx)) and rows likewise; every box has one
representative source pixel and every plane takes that pixel's value unchanged.
  POINT    (min(W-1, ox*fx + fx//2), min(H-1, oy*fy + fy//2))
  NEAREST  the box pixel with the smallest distance as a signed int16; ties: the lowest row, then the lowest column.
representatives() returns the chosen source coordinates, so that a test can say which pixel an implementation took."""
import numpy as np

POINT, NEAREST = 0, 1
NAMES = ("distance", "kind", "id", "cls")
DTYPES = {"distance": np.int16, "kind": np.uint8, "id": np.uint16, "cls": np.uint8}


def reduced_size(W, H, fx, fy):
    return -(-W // fx), -(-H // fy)


def representatives(rule, n, W, H, fx, fy, distance=None):
    """(ys, xs), each (n, oH, oW) int64: the representative source pixel of every box of every frame."""
    oW, oH = reduced_size(W, H, fx, fy)
    if rule == POINT:
        ys = np.minimum(H - 1, np.arange(oH) * fy + fy // 2)
        xs = np.minimum(W - 1, np.arange(oW) * fx + fx // 2)
        return np.broadcast_to(ys[None, :, None], (n, oH, oW)).copy(), np.broadcast_to(xs[None, None, :], (n, oH, oW)).copy()
    assert rule == NEAREST and distance is not None and distance.dtype == np.int16 and distance.shape == (n, H, W)
    far = np.int64(1) << 20                                             # a pixel that does not exist never wins: a box has one that does
    padded = np.full((n, oH * fy, oW * fx), far, dtype=np.int64)
    padded[:, :H, :W] = distance
    boxes = padded.reshape(n, oH, fy, oW, fx).transpose(0, 1, 3, 2, 4).reshape(n, oH, oW, fy * fx)   # each box row-major
    at = np.argmin(boxes, axis=3)                                       # the first minimum in row-major order: lowest row, then lowest column
    ys = np.arange(oH)[None, :, None] * fy + at // fx
    xs = np.arange(oW)[None, None, :] * fx + at % fx
    assert ys.max() < H and xs.max() < W
    return ys, xs


def reduce(rule, fx, fy, **planes):
    """planes: any of distance int16, kind uint8, id uint16, cls uint8, each (n, H, W) -> {name: (n, oH, oW)} of the same dtypes."""
    planes = {k: np.asarray(v) for k, v in planes.items() if v is not None}
    assert planes and set(planes) <= set(NAMES) and all(v.dtype == DTYPES[k] for k, v in planes.items())
    n, H, W = next(iter(planes.values())).shape
    ys, xs = representatives(rule, n, W, H, fx, fy, planes.get("distance"))
    f = np.arange(n)[:, None, None]
    return {k: v[f, ys, xs] for k, v in planes.items()}


# ---- the inputs both tiers run -------------------------------------------------------------------------------------------------------
CONTENTS = ["random", "equal", "last", "boxlast"]


def distance_content(kind, n, W, H, fx, fy, seed=0):
    """n distance planes (n, H, W) int16: seeded random over the full range with -32768 and 32767 present; all equal (every tie); 1000
    everywhere but -7 in the last row and column (edge boxes); each box's only minimum at its last pixel."""
    if kind == "random":
        d = np.random.default_rng([seed, W, H]).integers(-32768, 32768, size=(n, H, W), dtype=np.int64).astype(np.int16)
        flat = d.reshape(n, -1)
        flat[:, 0] = 32767                                               # (with one pixel the later write stands)
        flat[:, -1] = -32768
        return d
    if kind == "equal":
        return np.full((n, H, W), 1234, dtype=np.int16)
    if kind == "last":
        d = np.full((n, H, W), 1000, dtype=np.int16)
        d[:, H - 1, :] = -7
        d[:, :, W - 1] = -7
        return d
    if kind == "boxlast":
        y, x = np.mgrid[0:H, 0:W]
        d = (20000 - ((y % fy) * fx + (x % fx))).astype(np.int16)        # falls along the box's row-major order: the last pixel that exists is the smallest
        return np.broadcast_to(d, (n, H, W)).copy()
    raise ValueError(kind)


def tracer_planes(n, W, H):
    """id[y][x] = (y*W + x) & 0xFFFF, cls = id & 7, kind = (id >> 3) & 3: up to 65 536 pixels the id names its pixel, so an output says
    which source pixel was taken."""
    y, x = np.mgrid[0:H, 0:W]
    i = ((y * W + x) & 0xFFFF).astype(np.uint16)
    ids = np.broadcast_to(i, (n, H, W)).copy()
    return {"kind": ((ids >> 3) & 3).astype(np.uint8), "id": ids, "cls": (ids & 7).astype(np.uint8)}
