"""Numpy restatement of the box downscale (include/doomgpu.h: dg_reduce_desc), written from the contract's text:
oW = ceil(W / fx), oH = ceil(H / fy); output pixel (ox, oy) covers source columns [ox*fx, min(W, ox*fx + fx)) and rows likewise; per
channel out = floor((2*s + n) / (2*n)) with s the sum of the box's bytes and n its pixel count; gray = (77 r + 150 g + 29 b + 128) >> 8 of
the three rounded bytes.  Sums in int64."""
import numpy as np

RGB24, GRAY8 = 0, 1


def reduced_size(W, H, fx, fy, fmt=RGB24):
    oW, oH = -(-W // fx), -(-H // fy)
    return oW, oH, oW * oH * (1 if fmt == GRAY8 else 3)


def reduce(frames, fx, fy, fmt=RGB24):
    """frames (n, H, W, 3) uint8 -> (n, oH, oW, 3) uint8, or (n, oH, oW) as GRAY8."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    oW, oH, _ = reduced_size(W, H, fx, fy)
    padded = np.zeros((n, oH * fy, oW * fx, 3), dtype=np.int64)          # the pixels that do not exist add nothing to a sum
    padded[:, :H, :W] = frames
    s = padded.reshape(n, oH, fy, oW, fx, 3).sum(axis=(2, 4))
    ny = np.minimum(fy, H - np.arange(oH, dtype=np.int64) * fy)
    nx = np.minimum(fx, W - np.arange(oW, dtype=np.int64) * fx)
    cnt = (ny[:, None] * nx[None, :])[None, :, :, None]
    out = (2 * s + cnt) // (2 * cnt)
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    if fmt == GRAY8:
        out = (77 * out[..., 0] + 150 * out[..., 1] + 29 * out[..., 2] + 128) >> 8
    return out.astype(np.uint8)


# the grid both tiers run: (W, H), (fx, fy)
SIZES = [(64, 40), (80, 50), (131, 67), (5, 9), (1, 1), (320, 200)]
FACTORS = [(1, 1), (2, 2), (3, 3), (4, 5), (7, 3), (16, 16), (16, 1), (1, 16)]
CONTENTS = ["random", "zeros", "ones", "checker", "last"]


def content(kind, n, W, H, seed=0):
    """n frames (n, H, W, 3) uint8: seeded random bytes, all 0, all 255, a 0/255 checkerboard, only the last row and column 255."""
    if kind == "random":
        return np.random.default_rng([seed, W, H]).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    f = np.zeros((n, H, W, 3), dtype=np.uint8)
    if kind == "ones":
        f[:] = 255
    elif kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        f[:, (x + y) % 2 == 1] = 255
    elif kind == "last":
        f[:, H - 1, :] = 255
        f[:, :, W - 1] = 255
    elif kind != "zeros":
        raise ValueError(kind)
    return f
