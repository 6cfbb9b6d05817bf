"""Independent restatement of the player-centred map frames (include/doomgpu.h) in numpy / Python.

It reads VERTEXES and LINEDEFS itself (np_automap.read_map), keeps every value in f32 in the contract's operand order, floors with
np.floor, takes the arrow's trig from the host libm (doom_libm) and rasterises with np_automap.rasterise: the literal loop of SDL2's
RenderDrawLineBresenham.  Nothing here calls the product or shares code with ego_core.h.

Lines that start millions of pixels outside the frame (scale 64) would keep the literal loop busy for minutes before its first visible
point.  enter_frame() moves such a line's start to the last step before the frame's range along the major axis, with the loop's own state
there: after k steps the loop has added inc1 k - m times and inc2 m times, and its invariant inc2 <= d < inc1 (true at d0 = 2b - a,
kept by both branches when b <= a) leaves exactly one integer m.  From there on the loop runs literally (sdl_tail_points), and
test_ego_host.py holds the entry against the whole literal loop on lines short enough to run.
"""
from __future__ import annotations

import numpy as np

import np_automap as na
from doom_libm import _libm

F = np.float32
RED, YELLOW = na.RED, na.YELLOW
PI = F(np.pi)
ROTATE, ARROW = 1, 2
LONG = 4096                        # lines with more steps than this enter the frame through enter_frame


def points(W: int, H: int, vx, vy, view, scale, rotate: bool):
    """The point rule for arrays of vertices (f32 element by element, as for one); view = (x, y, angle, cos_a, sin_a) in f32."""
    x, y, _, c, s = (F(t) for t in view)
    scale = F(scale)
    vx, vy = np.asarray(vx, dtype=F), np.asarray(vy, dtype=F)
    with np.errstate(all="ignore"):
        dx, dy = vx - x, vy - y
        if rotate:
            r = dx * s - dy * c
            f = dx * c + dy * s
        else:
            r, f = dx, dy
        X = np.floor(F(W // 2) + r * scale)
        Y = np.floor(F(H // 2) - f * scale)
    assert X.dtype == F and Y.dtype == F
    return X.astype(np.int64), Y.astype(np.int64)


def point(W: int, H: int, vx, vy, view, scale, rotate: bool):
    X, Y = points(W, H, [vx], [vy], view, scale, rotate)
    return int(X[0]), int(Y[0])


def arrow(W: int, H: int, view, scale, rotate: bool):
    x, y, a, c, s = (F(t) for t in view)
    scale = F(scale)
    zero = F(0.0)
    ln, al = F(F(F(W) / F(16.0)) / scale), F(F(F(W) / F(32.0)) / scale)

    def rot(lx, ang_c, ang_s):
        return F(F(lx * ang_c) - F(zero * ang_s)), F(F(zero * ang_c) + F(lx * ang_s))

    with np.errstate(all="ignore"):
        dx, dy = rot(ln, c, s)
        ex, ey = F(x + dx), F(y + dy)
        ar, al_ = F(F(a - PI) - F(PI / F(4.0))), F(F(a - PI) + F(PI / F(4.0)))
        rdx, rdy = rot(al, F(_libm.cosf(ar)), F(_libm.sinf(ar)))
        ldx, ldy = rot(al, F(_libm.cosf(al_)), F(_libm.sinf(al_)))
        P = point(W, H, x, y, view, scale, rotate)
        E = point(W, H, ex, ey, view, scale, rotate)
        R = point(W, H, F(ex + rdx), F(ey + rdy), view, scale, rotate)
        L = point(W, H, F(ex + ldx), F(ey + ldy), view, scale, rotate)
    return [(*P, *E, YELLOW), (*R, *E, YELLOW), (*L, *E, YELLOW)]


def enter_frame(line, W: int, H: int):
    """(x, y, d, steps left, the loop's constants) of the literal loop at the last step before the frame's range along the line's major
    axis (step 0 when the line starts inside it), or None when that range is never reached."""
    x0, y0, x1, y1, _ = line
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xm = dx >= dy
    a, b = (dx, dy) if xm else (dy, dx)
    inc1, inc2 = 2 * b, 2 * (b - a)
    sx, sy = (-1 if x0 > x1 else 1), (-1 if y0 > y1 else 1)
    M0, N, sM = (x0, W, sx) if xm else (y0, H, sy)
    # steps k with 0 <= M0 + sM * k < N
    lo, hi = (-M0, N - 1 - M0) if sM > 0 else (M0 - (N - 1), M0)
    lo, hi = max(lo, 0), min(hi, a)
    if hi < lo:
        return None
    k = max(lo - 1, 0)
    m = 0
    if k and a:
        # d_k = d0 + inc1 * (k - m) + inc2 * m = d0 + 2 b k - 2 a m must lie in [inc2, inc1)
        d0 = 2 * b - a
        m = -((inc1 - 1 - d0 - 2 * b * k) // (2 * a))          # the smallest m with d_k <= inc1 - 1
        assert inc2 <= d0 + 2 * b * k - 2 * a * m < inc1
    d = 2 * b - a + 2 * b * k - 2 * a * m
    x, y = (x0 + sx * k, y0 + sy * m) if xm else (x0 + sx * m, y0 + sy * k)
    return x, y, d, hi - k + 1, (xm, inc1, inc2, sx, sy)


def sdl_tail_points(x, y, d, n, consts):
    """The literal loop from a state on: n points."""
    xm, inc1, inc2, sx, sy = consts
    out = []
    for _ in range(n):
        out.append((x, y))
        if d < 0:
            d += inc1
            x, y = (x + sx, y) if xm else (x, y + sy)
        else:
            d += inc2
            x, y = x + sx, y + sy
    return out


def rasterise(lines, W: int, H: int) -> np.ndarray:
    """np_automap.rasterise, with every long line replaced by its points from enter_frame on as one-point lines (same order, same colour:
    the same frame)."""
    flat = []
    for ln in lines:
        if max(abs(ln[2] - ln[0]), abs(ln[3] - ln[1])) <= LONG:
            flat.append(ln)
            continue
        st = enter_frame(ln, W, H)
        if st is None:
            continue
        flat += [(x, y, x, y, ln[4]) for x, y in sdl_tail_points(*st) if 0 <= x < W and 0 <= y < H]
    return na.rasterise(flat, W, H)


class EgoModel:
    def __init__(self, wad: bytes, map_name: str = "E1M1"):
        self.verts, self.lines = na.read_map(wad, map_name)
        self.n_lines = len(self.lines)
        self.words = (self.n_lines + 31) // 32

    def bits_to_row(self, lines) -> np.ndarray:
        row = np.zeros(self.words, dtype=np.uint32)
        for l in lines:
            row[int(l) >> 5] |= np.uint32(1 << (int(l) & 31))
        return row

    def lines_for(self, W: int, H: int, view, scale, flags: int, mask_row=None):
        """Draw-order lines [(x0, y0, x1, y1, rgb)] of one frame."""
        rot = bool(flags & ROTATE)
        keep = [l for l, (_, _, fl) in enumerate(self.lines)
                if not fl & 128 and (mask_row is None or (int(mask_row[l >> 5]) >> (l & 31)) & 1)]
        out = []
        if keep:
            v1 = [self.lines[l][0] for l in keep]
            v2 = [self.lines[l][1] for l in keep]
            vx, vy = np.array([v[0] for v in self.verts], F), np.array([v[1] for v in self.verts], F)
            X0, Y0 = points(W, H, vx[v1], vy[v1], view, scale, rot)
            X1, Y1 = points(W, H, vx[v2], vy[v2], view, scale, rot)
            out = [(int(X0[k]), int(Y0[k]), int(X1[k]), int(Y1[k]), YELLOW if self.lines[l][2] & 4 else RED) for k, l in enumerate(keep)]
        if flags & ARROW:
            out += arrow(W, H, view, scale, rot)
        return out

    def frame(self, W: int, H: int, view, scale, flags: int, mask_row=None) -> np.ndarray:
        return rasterise(self.lines_for(W, H, view, scale, flags, mask_row), W, H)


def view_of(v):
    """A ctypes dg_view (trig filled) as the model's 5-tuple."""
    return (F(v.x), F(v.y), F(v.angle), F(v.cos_a), F(v.sin_a))
