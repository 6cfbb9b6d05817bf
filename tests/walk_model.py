"""Model of the player movement from recorded keys (dg_walk_*), written from the reference's
Game::process_down_keys / update_current_player_height (src/game.rs:314-389) and get_sector_from_vertex (src/renderer/bsp.rs:9-44).
It shares no code with the product: the tic step is restated in numpy f32 with the cosf / sinf of tests/doom_libm.py, and the
descent reads the WAD's own NODES / SSECTORS / SEGS / LINEDEFS / SIDEDEFS / SECTORS lumps.

Two integrators: `walk` is the literal one, tic by tic; `straight_probes` covers walks whose keys never turn (the angle stays put,
so every move adds or subtracts one of four constant deltas) with one sequential f32 accumulate — it is what lets the CPU tier
check the inputs of the GPU tier, millions of probes, in seconds.  tests/test_walk_host.py checks the two against each other."""
import struct

import numpy as np

import doom_libm

LEFT, RIGHT, UP, DOWN, ALT, SHIFT = 1, 2, 4, 8, 16, 32
F = np.float32
PI = F(np.pi)


def cosf(a):
    return F(doom_libm._libm.cosf(float(a)))


def sinf(a):
    return F(doom_libm._libm.sinf(float(a)))


def _lumps(wad: bytes, map_name: str):
    n, diro = struct.unpack_from("<ii", wad, 4)
    names = [wad[diro + 16 * i + 8:diro + 16 * i + 16].rstrip(b"\0").decode("ascii").upper() for i in range(n)]
    at = names.index(map_name.upper())
    out = {}
    for want in ("THINGS", "LINEDEFS", "SIDEDEFS", "VERTEXES", "SEGS", "SSECTORS", "NODES", "SECTORS"):
        i = names.index(want, at + 1)
        off, size = struct.unpack_from("<ii", wad, diro + 16 * i)
        out[want] = wad[off:off + size]
    return out


class Bsp:
    """The map's BSP and, per subsector, the floor height get_sector_from_vertex would report (None flag: no seg with a sidedef)."""

    def __init__(self, wad: bytes, map_name: str = "E1M1", fused: bool = False):
        self.fused = fused                                                 # test code only: the side test as a contracting compiler would evaluate it (floor_at)
        L = _lumps(wad, map_name)
        nodes = np.frombuffer(L["NODES"], dtype="<i2").reshape(-1, 14)
        self.nx, self.ny, self.ndx, self.ndy = (nodes[:, k].astype(F) for k in range(4))
        self.child = nodes[:, 12:14].astype(np.int64) & 0xFFFF             # [:, 0] right, [:, 1] left
        segs = np.frombuffer(L["SEGS"], dtype="<i2").reshape(-1, 6)
        ssec = np.frombuffer(L["SSECTORS"], dtype="<i2").reshape(-1, 2)
        lines = np.frombuffer(L["LINEDEFS"], dtype="<i2").reshape(-1, 7)
        sides = np.frombuffer(L["SIDEDEFS"], dtype=np.uint8).reshape(-1, 30)
        sectors = np.frombuffer(L["SECTORS"], dtype=np.uint8).reshape(-1, 26)
        floor_of_sector = sectors[:, 0:2].copy().view("<i2")[:, 0]
        sector_of_side = sides[:, 28:30].copy().view("<i2")[:, 0]
        self.leaf_floor = np.zeros(len(ssec), dtype=F)
        self.leaf_none = np.ones(len(ssec), dtype=bool)
        for l, (count, first) in enumerate(ssec):
            for s in segs[first:first + count]:
                side = lines[s[3], 6] if s[4] else lines[s[3], 5]          # direction != 0: the back sidedef
                if side != -1:
                    self.leaf_floor[l] = F(floor_of_sector[sector_of_side[side]])
                    self.leaf_none[l] = False
                    break
        things = np.frombuffer(L["THINGS"], dtype="<i2").reshape(-1, 5)
        p1 = [t for t in things if t[3] == 1]
        self.start = (F(p1[0][0]), F(p1[0][1]), F(p1[0][2]) * (PI / F(180))) if p1 else None

    def floor_at(self, xs, ys):
        """-> (hit, floor) arrays: the sector's floor height where the point is in a sector."""
        xs = np.asarray(xs, dtype=F).reshape(-1)
        ys = np.asarray(ys, dtype=F).reshape(-1)
        cur = np.full(xs.size, len(self.nx) - 1, dtype=np.int64)
        leaf = np.zeros(xs.size, dtype=np.int64)
        live = np.arange(xs.size)
        with np.errstate(all="ignore"):
            while live.size:
                n = cur[live]
                x, y, dx, dy = self.nx[n], self.ny[n], self.ndx[n], self.ndy[n]
                ax, ay = xs[live] - x, ys[live] - y
                bx, by = (x + dx) - x, (y + dy) - y
                if self.fused:                                             # fma(ax, by, -(ay * bx)): the first product exact, one rounding of the sum
                    left = (ax.astype(np.float64) * by.astype(np.float64) - (ay * bx).astype(np.float64)).astype(F) <= F(0)
                else:
                    left = (ax * by - ay * bx) <= F(0)
                c = self.child[n, left.astype(np.int64)]
                is_leaf = (c & 0x8000) != 0
                leaf[live[is_leaf]] = c[is_leaf] & 0x7FFF
                cur[live] = c
                live = live[~is_leaf]
        return ~self.leaf_none[leaf], self.leaf_floor[leaf]


def lengths(turbo: int, shift: bool):
    duration = F(1000.0) / F(35.0)
    rotate_factor = duration * F(0.0025)
    move_factor = duration * F(0.291)
    turbo_f = F(turbo) / F(100.0)
    ml, ra = move_factor * turbo_f, rotate_factor * turbo_f
    if shift:
        ml, ra = ml * F(2.0), ra * F(2.0)
    return ml, ra


def rotate(x, angle):
    """Vertex::new(x, 0.0).rotate(angle), both terms kept."""
    c, s = cosf(angle), sinf(angle)
    with np.errstate(all="ignore"):
        return x * c - F(0.0) * s, F(0.0) * c + x * s


class Result:
    pass


def walk(bsp: Bsp, start, turbo: int, keys):
    """The literal model.  start: (x, y, angle) or None for Player1Start.  -> Result with pose (n + 1, 3) f32, floors (n + 1) f32,
    probes (list of (x, y)), end_of_tic, and sticky: the tics in which a mid-tic probe hit and the tic's last probe missed."""
    x, y, a = (F(v) for v in (bsp.start if start is None else start))
    r = Result()
    probes = [(x, y)]
    tic_of_probe = [0]
    pose = [(x, y, a)]
    end = [0]
    with np.errstate(all="ignore"):
        for t, k in enumerate(keys):
            k = int(k)
            alt = bool(k & ALT)
            ml, ra = lengths(turbo, bool(k & SHIFT))
            if not alt and k & LEFT:
                a = a + ra
            if not alt and k & RIGHT:
                a = a - ra
            if alt and k & LEFT:
                dx, dy = rotate(ml, a + PI / F(2.0))
                x, y = x + dx, y + dy
                probes.append((x, y)); tic_of_probe.append(t + 1)
            if alt and k & RIGHT:
                dx, dy = rotate(ml, a + PI / F(2.0))
                x, y = x - dx, y - dy
                probes.append((x, y)); tic_of_probe.append(t + 1)
            if k & UP:
                dx, dy = rotate(ml, a)
                x, y = x + dx, y + dy
                probes.append((x, y)); tic_of_probe.append(t + 1)
            if k & DOWN:
                dx, dy = rotate(ml, a)
                x, y = x - dx, y - dy
                probes.append((x, y)); tic_of_probe.append(t + 1)
            pose.append((x, y, a))
            end.append(len(probes) - 1)
    hit, fl = bsp.floor_at([p[0] for p in probes], [p[1] for p in probes])
    floors, cur, i = [], F(0.0), 0
    sticky = []
    for t, e in enumerate(end):
        mid_hit = False
        for j in range(i, e + 1):
            if hit[j]:
                cur = fl[j]
                mid_hit = mid_hit or j < e
        if e >= i and mid_hit and not hit[e]:
            sticky.append(t)
        i = e + 1
        floors.append(cur)
    r.pose = np.array(pose, dtype=F).reshape(-1, 3)
    r.floors = np.array(floors, dtype=F)
    r.probes, r.end_of_tic, r.hit, r.sticky = probes, end, hit, sticky
    return r


def tics_of(ts) -> int:
    """Clock::ticks: (timestamp * 35.0f32) as u32 (saturating, NaN and <= 0: 0)."""
    with np.errstate(all="ignore"):
        t = F(ts) * F(35.0)
    if not t > 0:
        return 0
    return 0xFFFFFFFF if t >= F(4294967296.0) else int(t)


def views(r: Result, timestamps):
    """(n, 10) rows: x, y, angle, floor, cos, sin, cos(-a), sin(-a), timestamp as f32 bits kept in a float32 column, and the tic."""
    out = np.zeros((len(timestamps), 10), dtype=F)
    n = len(r.floors) - 1
    for i, ts in enumerate(timestamps):
        t = min(tics_of(ts), n)
        x, y, a = r.pose[t]
        out[i] = (x, y, a, r.floors[t], cosf(a), sinf(a), cosf(-a), sinf(-a), F(ts), t)
    return out


def moves_of(keys):
    """Per tic the moves that run, in order: (sign, strafe, shift) for each; a mask that turns is refused."""
    moves, per_tic = [], []
    for k in keys:
        k = int(k)
        alt, sh = bool(k & ALT), bool(k & SHIFT)
        assert alt or not k & (LEFT | RIGHT), "straight walks do not turn"
        m = []
        if alt and k & LEFT:
            m.append((1, 1, sh))
        if alt and k & RIGHT:
            m.append((-1, 1, sh))
        if k & UP:
            m.append((1, 0, sh))
        if k & DOWN:
            m.append((-1, 0, sh))
        moves += m
        per_tic.append(len(m))
    return moves, per_tic


# probes per tic of a key mask that does not turn, and the (sign, strafe, shift) of each as indices into a delta table
_MOVE_TABLE = {}
for _k in range(64):
    if not (_k & ALT) and _k & (LEFT | RIGHT):
        continue
    _MOVE_TABLE[_k] = moves_of([_k])[0]


def straight_probes(start, turbo: int, keys):
    """The probes (x, y arrays, the start first) and end_of_tic of a walk whose keys never turn, by one sequential f32 accumulate."""
    x0, y0, a = (F(v) for v in start)
    keys = np.asarray(keys, dtype=np.uint8).reshape(-1)
    delta = np.zeros((2, 2, 2, 2), dtype=F)                   # [negative][strafe][shift] -> (dx, dy)
    for strafe in (0, 1):
        for sh in (0, 1):
            ml, _ = lengths(turbo, bool(sh))
            dx, dy = rotate(ml, a + PI / F(2.0) if strafe else a)
            delta[0, strafe, sh] = (dx, dy)
            delta[1, strafe, sh] = (-dx, -dy)                 # pos - d == pos + (-d) in IEEE arithmetic
    count = np.zeros(64, dtype=np.int64)
    code = np.zeros((64, 4), dtype=np.int64)                  # per mask its moves as flat indices into delta
    for k, mv in _MOVE_TABLE.items():
        count[k] = len(mv)
        for j, (sign, strafe, sh) in enumerate(mv):
            code[k, j] = (0 if sign > 0 else 4) + 2 * strafe + int(sh)
    k6 = keys & 63
    assert all(int(k) in _MOVE_TABLE for k in np.unique(k6)), "straight walks do not turn"
    per_tic = count[k6]
    slot = np.arange(4)[None, :] < per_tic[:, None]
    flat = code[k6][slot]                                     # row-major: tic by tic, move by move
    d = delta.reshape(8, 2)[flat]
    with np.errstate(all="ignore"):
        xs = np.add.accumulate(np.concatenate([[x0], d[:, 0]]).astype(F), dtype=F)
        ys = np.add.accumulate(np.concatenate([[y0], d[:, 1]]).astype(F), dtype=F)
    end = np.concatenate([[0], np.cumsum(per_tic)])
    return xs, ys, end


def floors_from_probes(bsp: Bsp, xs, ys, end):
    """floor[t] for one walk from its probes: the last hit at or before end[t], 0.0 before the first."""
    hit, fl = bsp.floor_at(xs, ys)
    idx = np.where(hit, np.arange(hit.size), -1)
    last = np.maximum.accumulate(idx)
    at = last[end]
    return np.where(at >= 0, fl[np.maximum(at, 0)], F(0.0)).astype(F), hit
