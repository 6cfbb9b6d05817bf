"""GPU tier of what the three 2-D map kinds share: one slot taken by a map, an explored and a player-centred submission in turn, the
state each leaves there for dg_replay_slot, and the per-scene tables across a second dg_upload_scene.

Every frame is held against the host rule byte for byte: dg_explored_map_host with all ones for the map view, dg_explored_map_host with
the rows for explored frames, dg_ego_map_host for player-centred frames.  64x40 is one band and the 16-byte store form of every kind; the
other store forms are test_automap_gpu.py's, test_explored_gpu.py's and test_ego_gpu.py's.
"""
import numpy as np
import pytest

import np_explored as ne

pytestmark = pytest.mark.gpu

W, H, N = 64, 40, 4


class Kinds:
    """One ctx and one scene: submissions of each kind into a slot, each checked against the host rule, its replay and its timing."""

    def __init__(self, dg, ctx, path):
        self.dg, self.ctx = dg, ctx
        self.views = dg.make_views(path[[0, 297, 500, 728]])
        self.built = set()                                  # kinds whose per-scene table this scene has had built
        self.fallbacks = ctx.fallbacks()

    def scene(self, sc, wad, seed):
        self.sc = sc
        model = ne.Explored(wad)
        assert model.words == self.dg.seen_words(sc)
        self.ones = np.tile(model.bits_to_row(range(model.n_lines)), (N, 1))
        self.rng = np.random.default_rng(seed)
        self.built = set()

    def rows(self):
        return self.rng.integers(0, 1 << 32, self.ones.shape, dtype=np.uint64).astype(np.uint32) & self.ones

    def host(self, kind, rows=None, params=None):
        dg = self.dg
        if kind == dg.DG_FE_MAP_EGO:
            return np.stack([dg.ego_map_host(self.sc, W, H, v, params, None if rows is None else rows[k]) for k, v in enumerate(self.views)])
        rows = self.ones if kind == dg.DG_FE_MAP else rows
        return np.stack([dg.explored_map_host(self.sc, W, H, v, rows[k]) for k, v in enumerate(self.views)])

    def submit(self, slot, kind, rows=None, params=None):
        dg, ctx = self.dg, self.ctx
        if kind == dg.DG_FE_MAP:
            ctx.submit_map(slot, self.views)
        elif kind == dg.DG_FE_MAP_EXPLORED:
            ctx.submit_explored_map(slot, self.views, rows)
        else:
            ctx.submit_ego_map(slot, self.views, params, rows)

    def step(self, slot, kind, rows=None, params=None):
        """Submit, compare with the host rule, replay, look at the timing; returns the frames."""
        ctx = self.ctx
        self.submit(slot, kind, rows, params)
        got = ctx.readback(slot, 0, N)
        want = self.host(kind, rows, params)
        for f in range(N):
            assert np.array_equal(got[f], want[f]), (kind, f, int((got[f] != want[f]).any(axis=2).sum()))
        t = ctx.timing(slot)
        assert t["front_end"] == kind and t["n_frames"] == N and t["raster_ms"] > 0
        assert (t["setup_ms"] > 0) == (kind not in self.built), (kind, t)       # the first submission of a kind builds its table
        self.built.add(kind)
        sums = list(ctx.frame_checksums(slot, 0, N))
        assert sums == [self.dg.frame_checksum(f) for f in want]
        ctx.replay(slot)
        assert list(ctx.frame_checksums(slot, 0, N)) == sums
        t = ctx.timing(slot)
        assert t["front_end"] == kind and t["setup_ms"] == 0.0                   # (the replay found the table there)
        assert ctx.fallbacks() == self.fallbacks
        return got


def test_three_kinds_through_one_slot(dg, wad1993, wad1995, path1993):
    MAP, EXPLORED, EGO = dg.DG_FE_MAP, dg.DG_FE_MAP_EXPLORED, dg.DG_FE_MAP_EGO
    sc = dg.Scene(wad1993, "e1m1")
    ctx = dg.Context(W, H, max_batch=N, slots=2)
    ctx.upload_scene(sc)
    k = Kinds(dg, ctx, path1993)
    k.scene(sc, wad1993, 1)
    frames = k.step(0, MAP)
    assert frames.any()
    k.step(0, EXPLORED, k.rows())
    k.step(0, EGO, k.rows(), (0.25, dg.DG_EGO_ROTATE | dg.DG_EGO_ARROW))
    k.step(0, EGO, None, (0.25, 0))                       # no mask after a mask, no arrow after an arrow
    a = k.step(0, EXPLORED, k.ones)
    b = k.step(0, MAP)
    assert np.array_equal(a, b)

    # the mask rows are the slot's: another slot's submission with other rows does not show in a replay
    rows1, rows0 = k.rows(), k.rows()
    assert not np.array_equal(rows0, rows1)
    kept = k.step(1, EXPLORED, rows1)
    k.step(0, EGO, rows0, (1.0, dg.DG_EGO_ARROW))
    ctx.replay(1)
    assert np.array_equal(ctx.readback(1, 0, N), kept)

    # a second scene: every per-scene table and the slots' mask rows are gone; the first submission comes without a mask
    sc2 = dg.Scene(wad1995, "e1m1")
    ctx.upload_scene(sc2)
    k.scene(sc2, wad1995, 2)
    k.step(0, EGO, None, (0.25, dg.DG_EGO_ROTATE | dg.DG_EGO_ARROW))
    k.step(0, EXPLORED, k.rows())
    k.step(0, MAP)
    assert ctx.fallbacks() == k.fallbacks
    ctx.close()
    sc2.close()
    sc.close()
