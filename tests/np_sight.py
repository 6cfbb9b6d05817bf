"""The line-of-sight rule restated twice in numpy float32, both from the map's lumps as the WAD holds them:

  model_a   the rule as the library states it: the BSP leaves a sight line visits, then every seg of those leaves
  model_b   the brute-force rule: the same per-linedef steps over EVERY linedef of the map, no BSP

Both evaluate every step of every query (no early exit: each step is a max into lo, a min into hi or an OR into a block flag, so the
order and an early exit cannot matter) and are vectorised over the queries.  float32 arrays make numpy round every operation to f32,
never fused; `/` is the correctly rounded division.

A query array has the fields of SIGHT_QUERY_DTYPE (frame, x0, y0, z0, x1, y1, z1_lo, z1_hi).  `heights`: int array (frames, sectors, 2)
of (floor, ceiling) — height_rows() builds it from the SECTORS lump and per-frame entries, later entries winning.

Outcomes: VISIBLE, ONE_SIDED (a one-sided linedef blocked), CLOSED (a two-sided linedef whose opening is closed blocked, or the slopes
crossed: hi <= lo), OUT (a field out of contract).  The library only reports VISIBLE or not.
"""
import struct

import numpy as np

F = np.float32
VISIBLE, ONE_SIDED, CLOSED, OUT = 0, 1, 2, 3
MAX_COORD = 65536.0
QUERY_DTYPE = np.dtype([("frame", "<i4"), ("x0", "<f4"), ("y0", "<f4"), ("z0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("z1_lo", "<f4"), ("z1_hi", "<f4")])


def _lump(wad: bytes, map_name: str, name: str) -> bytes:
    n, diro = struct.unpack_from("<ii", wad, 4)
    names = [wad[diro + 16 * i + 8:diro + 16 * i + 16].rstrip(b"\0").decode("ascii").upper() for i in range(n)]
    i = names.index(name, names.index(map_name.upper()) + 1)
    off, size = struct.unpack_from("<ii", wad, diro + 16 * i)
    return wad[off:off + size]


def queries(rows) -> np.ndarray:
    """rows of (frame, x0, y0, z0, x1, y1, z1_lo, z1_hi) -> a query array (the floats rounded to f32)."""
    out = np.zeros(len(rows), dtype=QUERY_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(r)
    return out


class SightMap:
    def __init__(self, wad: bytes, map_name: str = "E1M1"):
        v = np.frombuffer(_lump(wad, map_name, "VERTEXES"), dtype="<i2").reshape(-1, 2)
        self.vx, self.vy = v[:, 0].astype(F), v[:, 1].astype(F)
        ld = np.frombuffer(_lump(wad, map_name, "LINEDEFS"), dtype="<i2").reshape(-1, 7).astype(np.int64)
        self.line_v1, self.line_v2, self.line_flags = ld[:, 0], ld[:, 1], ld[:, 2] & 0xFFFF
        sd = _lump(wad, map_name, "SIDEDEFS")
        side_sector = np.array([struct.unpack_from("<h", sd, 30 * i + 28)[0] for i in range(len(sd) // 30)] + [-1], dtype=np.int64)
        front = np.where(ld[:, 5] >= 0, ld[:, 5], -1)
        back = np.where(ld[:, 6] >= 0, ld[:, 6], -1)
        self.line_front, self.line_back = side_sector[front], side_sector[back]          # (index -1: the appended "no sidedef")
        sec = _lump(wad, map_name, "SECTORS")
        self.heights = np.array([struct.unpack_from("<hh", sec, 26 * i) for i in range(len(sec) // 26)], dtype=np.int64).reshape(-1, 2)
        sg = np.frombuffer(_lump(wad, map_name, "SEGS"), dtype="<i2").reshape(-1, 6).astype(np.int64)
        self.seg_line = sg[:, 3]
        ss = np.frombuffer(_lump(wad, map_name, "SSECTORS"), dtype="<i2").reshape(-1, 2).astype(np.int64)
        self.leaf_count, self.leaf_first = ss[:, 0], ss[:, 1]
        nd = _lump(wad, map_name, "NODES")
        self.n_nodes = len(nd) // 28
        self.node = np.array([struct.unpack_from("<hhhh", nd, 28 * i) for i in range(self.n_nodes)], dtype=np.int64).reshape(-1, 4).astype(F)
        self.child = np.array([struct.unpack_from("<HH", nd, 28 * i + 24) for i in range(self.n_nodes)], dtype=np.int64).reshape(-1, 2)   # [0] right, [1] left; bit 15: a leaf

    # ---- pieces ------------------------------------------------------------------------------------------------------------------
    def height_rows(self, n_frames: int, entries=None) -> np.ndarray:
        """(n_frames, sectors, 2): the SECTORS heights, with entries[f] = [(sector, floor, ceiling), ...] applied in order."""
        rows = np.repeat(self.heights[None], n_frames, axis=0).copy()
        for f, es in enumerate(entries or []):
            for s, fl, ce in es:
                rows[f, s] = (fl, ce)
        return rows

    def depth(self) -> int:
        d = np.zeros(self.n_nodes, dtype=np.int64)
        for i in range(self.n_nodes):
            d[i] = 1 + max(0 if c & 0x8000 else d[c] for c in self.child[i])
        return int(d[-1]) if self.n_nodes else 0

    @staticmethod
    def in_contract(q) -> np.ndarray:
        ok = np.ones(len(q), bool)
        for k in ("x0", "y0", "z0", "x1", "y1", "z1_lo", "z1_hi"):
            with np.errstate(invalid="ignore"):
                ok &= np.isfinite(q[k]) & (np.abs(q[k]) <= F(MAX_COORD))
        return ok

    @staticmethod
    def _cross(px, py, ax, ay, dx, dy):
        return (px - ax) * dy - (py - ay) * dx

    def visited_leaves(self, q):
        """(leaves, queries) bool: the leaves every query visits; and (queries,) bool: some cS or cE on the way was 0."""
        Q = len(q)
        n_leaves = len(self.leaf_count)
        at_node = np.zeros((self.n_nodes, Q), bool)
        at_leaf = np.zeros((n_leaves, Q), bool)
        zero = np.zeros(Q, bool)
        if self.n_nodes == 0:
            at_leaf[0] = True
            return at_leaf, zero
        at_node[-1] = True
        x0, y0, x1, y1 = q["x0"], q["y0"], q["x1"], q["y1"]
        for i in range(self.n_nodes - 1, -1, -1):
            here = at_node[i]
            if not here.any():
                continue
            nx, ny, ndx, ndy = self.node[i]
            bx, by = F(F(nx + ndx) - nx), F(F(ny + ndy) - ny)
            cS, cE = self._cross(x0, y0, nx, ny, bx, by), self._cross(x1, y1, nx, ny, bx, by)
            zero |= here & ((cS == 0) | (cE == 0))
            left = cS <= 0
            far_too = ~np.where(left, cE < 0, cE > 0)
            for side in (0, 1):
                near = left if side == 1 else ~left
                goes = here & (near | far_too)
                c = int(self.child[i, side])
                if c & 0x8000:
                    at_leaf[c & 0x7FFF] |= goes
                else:
                    at_node[c] |= goes
        return at_leaf, zero

    def line_step(self, line: int, q, heights, active, state):
        """The per-linedef steps of linedef `line` for the queries in `active`; state = dict(lo, hi, one_sided, closed, zero)."""
        if not active.any():
            return
        x0, y0, x1, y1, z0 = q["x0"], q["y0"], q["x1"], q["y1"], q["z0"]
        ax, ay, bx, by = self.vx[self.line_v1[line]], self.vy[self.line_v1[line]], self.vx[self.line_v2[line]], self.vy[self.line_v2[line]]
        dx, dy = x1 - x0, y1 - y0
        t1, t2 = self._cross(ax, ay, x0, y0, dx, dy), self._cross(bx, by, x0, y0, dx, dy)
        lx, ly = F(bx - ax), F(by - ay)
        u1, u2 = self._cross(x0, y0, ax, ay, lx, ly), self._cross(x1, y1, ax, ay, lx, ly)
        state["zero"] |= active & ((t1 == 0) | (t2 == 0) | (u1 == 0) | (u2 == 0))
        cross = active & (np.sign(t1) != np.sign(t2)) & (np.sign(u1) != np.sign(u2))
        if not cross.any():
            return
        fs, bs = int(self.line_front[line]), int(self.line_back[line])
        if not (self.line_flags[line] & 4) or fs < 0 or bs < 0:
            state["one_sided"] |= cross
            return
        fr = q["frame"]
        fh, fc = heights[fr, fs, 0].astype(F), heights[fr, fs, 1].astype(F)
        bh, bc = heights[fr, bs, 0].astype(F), heights[fr, bs, 1].astype(F)
        cross = cross & ~((fh == bh) & (fc == bc))
        top, bot = np.minimum(fc, bc), np.maximum(fh, bh)
        state["closed"] |= cross & (bot >= top)
        cross = cross & (bot < top)
        with np.errstate(all="ignore"):
            frac = u1 / (u1 - u2)
            narrow = cross & (frac > 0)
            lo_v, hi_v = (bot - z0) / frac, (top - z0) / frac
        up = narrow & (fh != bh)
        state["lo"] = np.where(up, np.maximum(state["lo"], lo_v), state["lo"]).astype(F)
        down = narrow & (fc != bc)
        state["hi"] = np.where(down, np.minimum(state["hi"], hi_v), state["hi"]).astype(F)

    def _start(self, q):
        Q = len(q)
        with np.errstate(all="ignore"):
            return dict(lo=(q["z1_lo"] - q["z0"]).astype(F), hi=(q["z1_hi"] - q["z0"]).astype(F), one_sided=np.zeros(Q, bool), closed=np.zeros(Q, bool),
                        zero=np.zeros(Q, bool))

    @staticmethod
    def _outcome(ok, state):
        with np.errstate(invalid="ignore"):
            shut = state["closed"] | ~(state["hi"] > state["lo"])
        return np.where(~ok, OUT, np.where(state["one_sided"], ONE_SIDED, np.where(shut, CLOSED, VISIBLE))).astype(np.int64)

    # ---- the two models ------------------------------------------------------------------------------------------------------------
    def model_a(self, q, heights, details: bool = False):
        """The outcome of every query by the rule; details: also (queries,) bool `zero` — some cS, cE, t1, t2, u1 or u2 it met was 0."""
        ok = self.in_contract(q)
        safe = q.copy()
        for k in ("x0", "y0", "z0", "x1", "y1", "z1_lo", "z1_hi"):
            safe[k] = np.where(ok, q[k], F(0))
        at_leaf, node_zero = self.visited_leaves(safe)
        state = self._start(safe)
        for leaf in range(len(self.leaf_count)):
            active = ok & at_leaf[leaf]
            for k in range(int(self.leaf_first[leaf]), int(self.leaf_first[leaf] + self.leaf_count[leaf])):
                self.line_step(int(self.seg_line[k]), safe, heights, active, state)
        out = self._outcome(ok, state)
        return (out, state["zero"] | node_zero) if details else out

    def model_b(self, q, heights, details: bool = False):
        """The outcome of every query over every linedef of the map."""
        ok = self.in_contract(q)
        safe = q.copy()
        for k in ("x0", "y0", "z0", "x1", "y1", "z1_lo", "z1_hi"):
            safe[k] = np.where(ok, q[k], F(0))
        state = self._start(safe)
        for line in range(len(self.line_v1)):
            self.line_step(line, safe, heights, ok.copy(), state)
        out = self._outcome(ok, state)
        return (out, state["zero"]) if details else out

    def visible(self, q, heights) -> np.ndarray:
        """What the library reports: uint8, 1 visible."""
        return (self.model_a(q, heights) == VISIBLE).astype(np.uint8)
