"""Independent restatement of the explored-map frames in numpy / Python: the seen rows of label planes, the running OR along a session,
and the map frame drawn through a line mask.

It reads SEGS and LINEDEFS itself (np_automap.read_map style: the first directory entry named like the map, + 5 / + 2) and draws with
np_automap's literal SDL loop.  Nothing here calls the product.
"""
from __future__ import annotations

import importlib
import struct

import numpy as np

import np_automap as na

sw = importlib.import_module("doom-rust-renderer_amd.synth_wad")

LABEL_WALL = 1


def read_seg_lines(wad: bytes, map_name: str = "E1M1") -> np.ndarray:
    """The linedef of every seg (SEGS entries are 12 bytes, the linedef is the fourth int16)."""
    d = sw.wad_directory(wad)
    i = next(k for k, (name, _, _) in enumerate(d) if name == map_name.upper())
    _, so, ss = d[i + 5]
    return np.array([ld for _, _, _, ld, _, _ in struct.iter_unpack("<hhhhhh", wad[so:so + ss - ss % 12])], dtype=np.int64)


class Explored:
    def __init__(self, wad: bytes, map_name: str = "E1M1"):
        self.mv = na.MapView(wad, map_name)
        self.seg_line = read_seg_lines(wad, map_name)
        self.n_lines = len(self.mv.lines)
        self.words = (self.n_lines + 31) // 32
        self._base = {}

    def bits_to_row(self, lines) -> np.ndarray:
        row = np.zeros(self.words, dtype=np.uint32)
        for l in lines:
            row[int(l) >> 5] |= np.uint32(1 << (int(l) & 31))
        return row

    def row_to_lines(self, row) -> list:
        return [l for l in range(self.n_lines) if (int(row[l >> 5]) >> (l & 31)) & 1]

    def seen(self, id, cls) -> np.ndarray:
        """(n, words) uint32: per frame the linedefs of the segs that own a wall pixel; ids at or beyond the seg count are ignored."""
        id, cls = np.asarray(id), np.asarray(cls)
        out = np.zeros((id.shape[0], self.words), dtype=np.uint32)
        for f in range(id.shape[0]):
            segs = np.unique(id[f][cls[f] == LABEL_WALL]).astype(np.int64)
            segs = segs[segs < len(self.seg_line)]
            out[f] = self.bits_to_row(np.unique(self.seg_line[segs]))
        return out

    def frame(self, W: int, H: int, view, mask_row) -> np.ndarray:
        """The map frame of `view` (np_automap's 5-tuple, or None: no arrow) with only the linedefs of mask_row."""
        lines, k = [], 0
        if (W, H) not in self._base:
            self._base[(W, H)] = self.mv.lines_for(W, H)
        base = self._base[(W, H)]
        for l, (_, _, fl) in enumerate(self.mv.lines):
            if fl & 128:
                continue
            if (int(mask_row[l >> 5]) >> (l & 31)) & 1:
                lines.append(base[k])
            k += 1
        if view is not None:
            lines += self.mv.arrow(W, H, *view)
        return na.rasterise(lines, W, H)


def popcount(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.uint32)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (4,)), axis=-1).sum(axis=(-1, -2)).astype(np.uint32)


def accumulate(seen, run_len: int, carry_in=None) -> dict:
    """upto, total, fresh, carry_out of the rows `seen` (n, words) taken as n / run_len runs."""
    seen = np.asarray(seen, dtype=np.uint32)
    n, words = seen.shape
    runs = n // run_len
    carry = np.zeros((runs, words), dtype=np.uint32) if carry_in is None else np.asarray(carry_in, dtype=np.uint32).reshape(runs, words)
    r = seen.reshape(runs, run_len, words).copy()
    r[:, 0, :] |= carry
    upto = np.bitwise_or.accumulate(r, axis=1)
    prev = np.concatenate([carry[:, None, :], upto[:, :-1, :]], axis=1)
    return {"upto": upto.reshape(n, words), "total": popcount(upto).reshape(n), "fresh": popcount(upto & ~prev).reshape(n),
            "carry_out": upto[:, -1, :].copy()}
