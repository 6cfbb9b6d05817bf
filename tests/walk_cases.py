"""Inputs shared by tests/test_walk_host.py and tests/test_walk_gpu.py: a map in which a point can be in no sector, and the walks of
the GPU tier's floor comparison.

get_sector_from_vertex (src/renderer/bsp.rs:9-44) reports None only for a subsector none of whose segs has a sidedef on its side —
the BSP's half-planes cover the whole plane, so on a well-formed map even a point far outside lands in a sector.  `holes_wad` empties
subsectors of a synthetic map (SSECTORS count 0): every subsector a far ring of points falls into, so that "far outside" misses, and
every seventh of the others, so that walks inside the map cross between hits and misses all the time.

`gpu_calls` builds, for every total probe count the GPU tier asks for, the walks of one dg_ctx_locate_walks call.  None of their keys
turn, so tests/walk_model.py can work out their probes by one accumulate and the CPU tier can check the mix (test_walk_host.py).

`line_walks` starts walks on the hand world's partition line: at the points where the side test is 0.0 and a fused one is not, and at
the exact ties on the partition, on segs and on vertices (tests/floor_map_cases.py finds both kinds).  Importing this module asserts,
by the model alone, that a fused side test puts four and more of those starts on the other room's floor."""
import struct

import numpy as np

import floor_map_cases as fc
import walk_model as wm

L, R, U, D, A, S = wm.LEFT, wm.RIGHT, wm.UP, wm.DOWN, wm.ALT, wm.SHIFT
FAR = 30000.0
# key masks that do not turn, with 0 .. 4 moves each (bits 6 and 7 are ignored by the product)
STRAIGHT = np.array([U, D, U | S, D | S, A | L, A | R, A | L | U, A | L | R | U | D, S, 0, A | R | D | S, 64 | U, 128 | D, A | L | R | D],
                    dtype=np.uint8)
TOTALS = [1, 2] + [(1 << k) + d for k in range(6, 22) for d in (-1, 0, 1)]


def far_ring(n=720):
    t = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    out = []
    for r in (FAR, 1.0e5):
        out.append(np.stack([2048.0 + r * np.cos(t), 1536.0 + r * np.sin(t)], axis=1))
    return np.concatenate(out).astype(np.float32)


def holes_wad(wad: bytes, map_name: str = "E1M1") -> bytes:
    n, diro = struct.unpack_from("<ii", wad, 4)
    names = [wad[diro + 16 * i + 8:diro + 16 * i + 16].rstrip(b"\0").decode("ascii").upper() for i in range(n)]
    i = names.index("SSECTORS", names.index(map_name.upper()) + 1)
    off, size = struct.unpack_from("<ii", wad, diro + 16 * i)
    bsp = wm.Bsp(wad, map_name)
    ring = far_ring()
    # the leaves of the ring's points: descend with every leaf marked by its own index
    probe = wm.Bsp(wad, map_name)
    probe.leaf_floor = np.arange(len(probe.leaf_floor), dtype=np.float32)
    probe.leaf_none[:] = False
    _, leaf = probe.floor_at(ring[:, 0], ring[:, 1])
    holes = set(int(v) for v in leaf) | set(range(0, len(bsp.leaf_floor), 7))
    out = bytearray(wad)
    for l in holes:
        struct.pack_into("<h", out, off + 4 * l, 0)
    return bytes(out)


def _keys_for(rng, moves: int) -> np.ndarray:
    """Straight masks whose moves add up to `moves` exactly: random ones, and for a long walk stretches of up to 6 000 random moves, each
    followed by its mirror image (forward for backward, left for right), so that the walk keeps coming back to where it was."""
    if moves <= 12000:
        return _random_keys(rng, moves)
    base = _random_keys(rng, 6000)
    mirror = (base & ~np.uint8(U | D | L | R)) | np.where(base & U, D, 0).astype(np.uint8) | np.where(base & D, U, 0).astype(np.uint8) \
        | np.where(base & L, R, 0).astype(np.uint8) | np.where(base & R, L, 0).astype(np.uint8)
    there_and_back = np.concatenate([base, mirror])
    return np.concatenate([np.tile(there_and_back, moves // 12000), _random_keys(rng, moves % 12000)])


def _random_keys(rng, moves: int) -> np.ndarray:
    if moves == 0:
        return np.zeros(0, dtype=np.uint8)
    count = np.array([len(wm._MOVE_TABLE[int(k) & 63]) for k in STRAIGHT])
    pick = rng.integers(0, len(STRAIGHT), moves + 8)
    cum = np.cumsum(count[pick])
    keep = int(np.searchsorted(cum, moves, side="right"))
    rest = moves - (int(cum[keep - 1]) if keep else 0)
    return np.concatenate([STRAIGHT[pick[:keep]], np.full(rest, U, dtype=np.uint8)])


def _sizes(total: int, rng):
    """Walk sizes (probes) of one call: boundaries on every 2^k - 1, 2^k, 2^k + 1 below the total, a zero-tic walk first, and a
    few random boundaries."""
    cuts = {1} | {(1 << k) + d for k in range(6, 22) for d in (-1, 0, 1)}
    cuts |= set(int(v) for v in rng.integers(1, max(2, total), 6))
    cuts = sorted(c for c in cuts if 0 < c < total) + [total]
    return [b - a for a, b in zip([0] + cuts[:-1], cuts)]


def gpu_calls(bsp):
    """-> [(total, [(start, turbo, keys), ...]), ...] for every total of TOTALS.  bsp: the model's view of the map (wm.Bsp of holes_wad);
    it is only asked where a walk of 64 probes or more may start so that it starts in a sector."""
    calls = []
    for total in TOTALS:
        rng = np.random.default_rng(2002 + total)
        descs = []
        for j, n in enumerate(_sizes(total, rng)):
            # far outside: a quarter of the short walks, and the walk that ends at 2^15 - 1 (16 382 probes: a run of misses beyond 2^13)
            far = (1 << 14) - 2 <= n < (1 << 15) or (n < 4096 and rng.random() < 0.25)
            if far:
                ang = rng.uniform(0.0, 2.0 * np.pi)
                start = (2048.0 + FAR * np.cos(ang), 1536.0 + FAR * np.sin(ang), rng.uniform(-3.0, 3.0))
            else:
                start = (rng.uniform(0.0, 4096.0), rng.uniform(0.0, 3072.0), rng.uniform(-3.0, 3.0))
                while n >= 64 and not bsp.floor_at([start[0]], [start[1]])[0][0]:
                    start = (rng.uniform(0.0, 4096.0), rng.uniform(0.0, 3072.0), start[2])
            start = tuple(float(np.float32(v)) for v in start)
            turbo = int(rng.choice([100, 255, 40] if n < 4096 else [20, 40, 60]))      # (a long walk wanders 77 steps from its start and back)
            descs.append((start, turbo, _keys_for(rng, n - 1)))
        calls.append((total, descs))
    return calls


def hand_wad() -> bytes:
    return fc.wad_of("hand")


def line_starts():
    """(xs, ys, n_witnesses): the witness points first, then the exact ties."""
    wx, wy = fc.side_witness_points()
    tx, ty = fc.tie_points()
    return np.concatenate([wx, tx]), np.concatenate([wy, ty]), len(wx)


def line_walks():
    """[(start, turbo, keys), ...] on the hand world: from every point of line_starts a walk of no tics and one of a few tics that
    steps off the line and back (its later probes land where they land: the model follows)."""
    xs, ys, _ = line_starts()
    out = []
    for i, (x, y) in enumerate(zip(xs, ys)):
        start = (float(x), float(y), float(np.float32(0.37 * i)))
        out.append((start, 100, np.zeros(0, dtype=np.uint8)))
        out.append((start, 40, np.array([U, D, A | L, A | R, 0, U | S][:2 + i % 5], dtype=np.uint8)))
    return out


def _line_starts_shown():
    xs, ys, n = line_starts()
    rule, fused = wm.Bsp(hand_wad()), wm.Bsp(hand_wad(), fused=True)
    (hit, floor), (fhit, ffloor) = rule.floor_at(xs, ys), fused.floor_at(xs, ys)
    assert hit.all() and fhit.all()
    other = (floor == 0.0) & (ffloor == 24.0)                 # room A's floor by the rule, room B's by a fused test
    assert other[:n].sum() >= 4 and other[:n].all(), int(other[:n].sum())
    assert not other[n:].any() and len(xs) - n >= 8           # an exact tie is one for a fused test too


_line_starts_shown()
