"""Independent restatement of the 2-D map view (the reference's `viewing_map` frame, src/game.rs:229-309, 491-499) in numpy / Python.

It reads VERTEXES and LINEDEFS itself (the first directory entry named like the map, + 4 / + 2: src/wad.rs:175-183), keeps every value
in f32 in the reference's operand order, takes the trig of the host libm (doom_libm) and rasterises with the literal loop of SDL2's
RenderDrawLineBresenham (draw_last = true), not the library's closed form.  Nothing here calls the product.
"""
from __future__ import annotations

import importlib
import struct

import numpy as np

from doom_libm import _libm

sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")

F = np.float32
RED, YELLOW = 0x0000FF, 0x00FFFF          # r | g << 8 | b << 16
PI = F(np.pi)                             # std::f32::consts::PI
LIMIT = 1 << 24


class OutOfContract(ValueError):
    pass


def read_map(wad: bytes, map_name: str = "E1M1"):
    """(vertices [(x, y) f32], linedefs [(v1, v2, flags)]) of the first map marker named map_name."""
    d = sw.wad_directory(wad)
    i = next(k for k, (name, _, _) in enumerate(d) if name == map_name.upper())
    _, lo, ls = d[i + 2]
    _, vo, vs = d[i + 4]
    verts = [(F(x), F(y)) for x, y in struct.iter_unpack("<hh", wad[vo:vo + vs - vs % 4])]
    lines = [(v1, v2, fl) for v1, v2, fl, _, _, _, _ in struct.iter_unpack("<hhhhhhh", wad[lo:lo + ls - ls % 14])]
    return verts, lines


def as_i32(f) -> int:
    """Rust `f as i32`: truncate toward zero, saturate, NaN -> 0."""
    f = float(f)
    if f != f:
        return 0
    if f <= -2147483648.0:
        return -2147483648
    if f >= 2147483647.0:
        return 2147483647
    return int(f)


class MapView:
    def __init__(self, wad: bytes, map_name: str = "E1M1"):
        self.verts, self.lines = read_map(wad, map_name)
        left = top = F(np.finfo(np.float32).max)
        right = bottom = F(np.finfo(np.float32).min)
        for v1, v2, _ in self.lines:                     # Map::new, src/map/mod.rs:59-64
            for x, y in (self.verts[v1], self.verts[v2]):
                left, right, top, bottom = min(left, x), max(right, x), min(top, y), max(bottom, y)
        self.left, self.right, self.top, self.bottom = left, right, top, bottom

    def point(self, W: int, H: int, x, y):
        """transform_vertex_to_point_for_map, game.rs:229-243."""
        with np.errstate(all="ignore"):
            xs, ys = F(self.right - self.left), F(self.bottom - self.top)
            sw_, sh, b = F(W - 40), F(H - 40), F(20.0)
            X = F(b + F(F(F(F(x) - self.left) * sw_) / xs))
            Y = F(F(F(b + sh) - F(1.0)) - F(F(F(F(y) - self.top) * sh) / ys))
        return as_i32(X), as_i32(Y)

    def lines_for(self, W: int, H: int, view=None):
        """Draw-order lines [(x0, y0, x1, y1, rgb)]; view = (x, y, angle, cos_a, sin_a) in f32, or None for the linedefs only."""
        if W < 40 or H < 40:
            raise OutOfContract("frame under 40 x 40")
        out = []
        for v1, v2, fl in self.lines:                    # draw_map_linedefs, game.rs:245-262
            if fl & 128:
                continue
            p0 = self.point(W, H, *self.verts[v1])
            p1 = self.point(W, H, *self.verts[v2])
            out.append((*p0, *p1, YELLOW if fl & 4 else RED))
        if view is not None:
            out += self.arrow(W, H, *view)
        return out

    def arrow(self, W: int, H: int, x, y, a, c, s):
        """draw_map_player, game.rs:287-309; Vertex::rotate evaluated literally."""
        x, y, a, c, s = F(x), F(y), F(a), F(c), F(s)
        ln, al = F(F(W) / F(16.0)), F(F(W) / F(32.0))
        zero = F(0.0)

        def rot(lx, ang_c, ang_s):
            return F(F(lx * ang_c) - F(zero * ang_s)), F(F(zero * ang_c) + F(lx * ang_s))

        with np.errstate(all="ignore"):
            dx, dy = rot(ln, c, s)
            ex, ey = F(x + dx), F(y + dy)
            ar, al_ = F(F(a - PI) - F(PI / F(4.0))), F(F(a - PI) + F(PI / F(4.0)))
            rdx, rdy = rot(al, F(_libm.cosf(ar)), F(_libm.sinf(ar)))
            ldx, ldy = rot(al, F(_libm.cosf(al_)), F(_libm.sinf(al_)))
            pts = [self.point(W, H, x, y), self.point(W, H, ex, ey), self.point(W, H, F(ex + rdx), F(ey + rdy)),
                   self.point(W, H, F(ex + ldx), F(ey + ldy))]
        if any(abs(v) > LIMIT for p in pts for v in p):
            raise OutOfContract("arrow beyond +-2^24")
        P, E, R, L = pts
        return [(*P, *E, YELLOW), (*R, *E, YELLOW), (*L, *E, YELLOW)]

    def render(self, W: int, H: int, view=None) -> np.ndarray:
        return rasterise(self.lines_for(W, H, view), W, H)


def sdl_line_points(x0, y0, x1, y1):
    """The literal loop of SDL2's RenderDrawLineBresenham with draw_last = true (every point, unclipped)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    if dx >= dy:
        n, d, inc1, inc2, xi1, xi2, yi1, yi2 = dx + 1, 2 * dy - dx, 2 * dy, 2 * (dy - dx), 1, 1, 0, 1
    else:
        n, d, inc1, inc2, xi1, xi2, yi1, yi2 = dy + 1, 2 * dx - dy, 2 * dx, 2 * (dx - dy), 0, 1, 1, 1
    if x0 > x1:
        xi1, xi2 = -xi1, -xi2
    if y0 > y1:
        yi1, yi2 = -yi1, -yi2
    x, y = x0, y0
    out = []
    for _ in range(n):
        out.append((x, y))
        if d < 0:
            d += inc1
            x += xi1
            y += yi1
        else:
            d += inc2
            x += xi2
            y += yi2
    return out


def _points_vectorised(lines):
    """The same loop, run for all lines at once (one numpy step per loop iteration): (line index, x, y) of every point."""
    L = np.asarray(lines, dtype=np.int64).reshape(-1, 5)
    x0, y0, x1, y1 = L[:, 0], L[:, 1], L[:, 2], L[:, 3]
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    xm = dx >= dy
    n = np.where(xm, dx, dy) + 1
    d = np.where(xm, 2 * dy - dx, 2 * dx - dy)
    inc1 = np.where(xm, 2 * dy, 2 * dx)
    inc2 = np.where(xm, 2 * (dy - dx), 2 * (dx - dy))
    sx = np.where(x0 > x1, -1, 1)
    sy = np.where(y0 > y1, -1, 1)
    xi1, yi1 = np.where(xm, sx, 0), np.where(xm, 0, sy)
    xi2, yi2 = sx, sy
    x, y = x0.copy(), y0.copy()
    idx, xs, ys = [], [], []
    for k in range(int(n.max()) if len(n) else 0):
        live = np.nonzero(n > k)[0]
        idx.append(live)
        xs.append(x[live].copy())
        ys.append(y[live].copy())
        neg = d < 0
        d = np.where(neg, d + inc1, d + inc2)
        x = x + np.where(neg, xi1, xi2)
        y = y + np.where(neg, yi1, yi2)
    if not idx:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(idx), np.concatenate(xs), np.concatenate(ys)


def rasterise(lines, W: int, H: int) -> np.ndarray:
    """(H, W, 3) uint8: black, then every line in order (points outside the frame dropped, a later line over an earlier one)."""
    img = np.zeros((H, W, 3), np.uint8)
    if not lines:
        return img
    idx, x, y = _points_vectorised(lines)
    keep = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    idx, pix = idx[keep], (y[keep] * W + x[keep])
    order = np.argsort(idx, kind="stable")
    idx, pix = idx[order], pix[order]
    last = np.unique(pix[::-1], return_index=True)[1]      # the last line to touch each pixel wins
    pix_u, line_u = pix[::-1][last], idx[::-1][last]
    rgb = np.asarray(lines, dtype=np.int64).reshape(-1, 5)[:, 4][line_u]
    flat = img.reshape(-1, 3)
    flat[pix_u, 0] = rgb & 255
    flat[pix_u, 1] = (rgb >> 8) & 255
    flat[pix_u, 2] = (rgb >> 16) & 255
    return img


def path_view(rec):
    """camera_path record [x, y, angle, cos, sin, cos(-a), sin(-a), floor] -> (x, y, angle, cos_a, sin_a)."""
    return (F(rec[0]), F(rec[1]), F(rec[2]), F(rec[3]), F(rec[4]))


def libm_view(x, y, angle):
    """A view with trig_valid = 0: the library takes cosf / sinf of the angle."""
    a = F(angle)
    return (F(x), F(y), a, F(_libm.cosf(a)), F(_libm.sinf(a)))


def patch_linedef_flags(wad: bytes, map_name: str, set_bits) -> bytes:
    """A copy of wad whose LINEDEFS entries k get flags |= bits for every (k, bits) in set_bits."""
    d = sw.wad_directory(wad)
    i = next(k for k, (name, _, _) in enumerate(d) if name == map_name.upper())
    _, lo, _ = d[i + 2]
    out = bytearray(wad)
    for k, bits in set_bits:
        o = lo + 14 * k + 4
        (fl,) = struct.unpack_from("<h", out, o)
        struct.pack_into("<h", out, o, fl | bits)
    return bytes(out)
