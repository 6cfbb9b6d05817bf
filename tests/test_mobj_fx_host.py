"""CPU tier of the map-object state machine (dg_scene_set_mobj_thinkers, DG_MOBJ_THINKERS): the model's orbit shortcut against its own
tic-by-tic run; dg_scene_mobj_states_at against the model at every tic up to 400 (far beyond twice the longest prefix + period), at the
f32 values just below and at each tic boundary, far out, at u32 saturation and for NaN / -0.0 / negative time; with event lists of each
kind, several in a row, at a state switch, at tic 0 and two at one tic; states of the longest tics an i16 holds; the precedence over
dg_scene_set_mobj_state; every error return; the host walker (dg_build_lists) with the setting on against a flags-0 scene given the
model's states; flags 0 after 1; and dg_mobj_rows' ISA budget."""
import ctypes
import os

import numpy as np
import pytest

import mobj_fx as mf

F32 = np.float32
VIEWS = list(range(0, 1000, 83))
N_TICS = 400

EVENT_LISTS = [
    [(mf.KILL, 30)],
    [(mf.EXPLODE, 30)],
    [(mf.RESPAWN, 17)],
    [(mf.KILL, 0)],                                               # at tic 0: before the first mutate
    [(mf.EXPLODE, 0), (mf.RESPAWN, 0)],                           # two at one tic: the later call acts last
    [(mf.KILL, 6)],                                               # exactly where BAR1 switches 1 -> 2
    [(mf.EXPLODE, 10), (mf.KILL, 13)],                            # exactly where TROO switches 6 -> 7 and 7 -> 8
    [(mf.KILL, 12), (mf.RESPAWN, 20), (mf.EXPLODE, 41), (mf.KILL, 41), (mf.RESPAWN, 90), (mf.EXPLODE, 95)],
    [(mf.KILL, 5), (mf.KILL, 9), (mf.KILL, 9), (mf.EXPLODE, 40), (mf.EXPLODE, 44), (mf.RESPAWN, 300)],
    [(1 + k % 3, 7 * k) for k in range(mf.MAX_EVENTS)],           # a full list
]


@pytest.fixture(scope="module")
def wad():
    return mf.fx_wad()


def _scene(dg, wad, states=mf.STATES, infos=mf.INFOS, events=()):
    sc = dg.Scene(wad, "E1M1")
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, states, infos)
    for what, E in events:
        sc.mobj_event(what, mf.ts(E))
    return sc


@pytest.fixture(scope="module")
def spawn_view(dg, wad):
    sc = dg.Scene(wad, "E1M1")
    out = sc.mobj_states_at(0.0)
    sc.close()
    return out


def _expect(sc, spawn_view, shown):
    """The model's `shown` list in the library's terms: (sprite_frame handle or -1, full_bright) per map object."""
    cache = sc.__dict__.setdefault("_handles", {})
    out = []
    for i, s in enumerate(shown):
        if s is None:
            out.append(spawn_view[i])
        elif s == "null":
            out.append((-1, 0))
        else:
            if s[:2] not in cache:
                cache[s[:2]] = sc.sprite_frame(s[0], s[1])
            out.append((cache[s[:2]], s[2]))
    return out


def test_fixture_has_what_the_contract_names(wad):
    sim = mf.Sim(wad)
    types = set(sim.types)
    assert {2035, 3001, 3004, 34, 2028, 2014, 46, 48}.issubset(types)                   # every case of the tables is in the map
    by_type = {t: d for t, d in zip(sim.types, sim.driven)}
    assert by_type[48] is False and by_type[2028] is False                              # no row; spawn chain not live
    assert all(by_type[t] for t in (2035, 3001, 3004, 34, 2014, 46))
    assert ("XXXX", 0) not in mf.sprite_frames_in(wad) and ("TROO", 3) in mf.sprite_frames_in(wad)
    assert sim.live(3) and sim.live(13) and not sim.live(22) and not sim.live(21)
    assert mf.ts(7) and mf.tics(mf.ts(7)) == 7
    assert N_TICS >= 2 * mf.LONGEST


def test_model_shortcut_equals_its_tic_by_tic_run(wad):
    class Short(mf.Sim):
        LIMIT = 45
    for ev in ([], EVENT_LISTS[7][:3]):
        a, b = mf.Sim(wad, events=ev), Short(wad, events=ev)
        for T in range(mf.Sim.LIMIT + 1):
            assert a.state_ids(T) == b.state_ids(T), T
    for start in (1, 3, 6, 10, 13, 15, 18, 20, 25, 27):
        w = mf.walk(mf.STATES, start, 100)
        sim = mf.Sim(wad, infos=[(3001, start, 0, 0)])
        i = sim.types.index(3001)
        assert [sim.state_ids(T)[i] for T in range(101)] == w, start


def test_states_at_every_tic(dg, wad, spawn_view):
    sim = mf.Sim(wad)
    sc = _scene(dg, wad)
    switched = 0
    for T in range(N_TICS + 1):
        want = _expect(sc, spawn_view, sim.shown(T))
        assert sc.mobj_states_at(mf.ts(T)) == want, T
        switched += want != spawn_view
    assert switched >= N_TICS * 9 // 10                                                 # (the spawn view is not what is being compared)
    sc.close()


def test_tic_boundaries_and_edge_timestamps(dg, wad, spawn_view):
    sim = mf.Sim(wad)
    sc = _scene(dg, wad)
    times = []
    for T in range(1, 64):
        t = F32(T / 35.0)
        while mf.tics(t) < T:
            t = np.nextafter(t, F32(np.inf))
        while mf.tics(np.nextafter(t, F32(-np.inf))) == T:
            t = np.nextafter(t, F32(-np.inf))
        assert mf.tics(t) == T and mf.tics(np.nextafter(t, F32(-np.inf))) == T - 1
        times += [float(np.nextafter(t, F32(-np.inf))), float(t)]
    times += [float(2.0 ** 24), 1e7, float(F32(2.0 ** 32 / 35.0)), 1e12, 3e38, float("inf"), float("nan"), -0.0, 0.0, -1.0, -1e30, float("-inf"), 1e-30]
    assert mf.tics(2.0 ** 24) == 35 * 2 ** 24 and mf.tics(1e12) == 2 ** 32 - 1 and mf.tics(float("nan")) == 0
    for t in times:
        assert sc.mobj_states_at(t) == _expect(sc, spawn_view, sim.shown(mf.tics(t))), t
    sc.close()


@pytest.mark.parametrize("k", range(len(EVENT_LISTS)))
def test_event_lists(dg, wad, spawn_view, k):
    ev = EVENT_LISTS[k]
    sim = mf.Sim(wad, events=ev)
    sc = _scene(dg, wad, events=ev)
    for T in list(range(N_TICS + 1)) + [mf.Sim.LIMIT, mf.Sim.LIMIT + 1, 99999]:
        assert sc.mobj_states_at(mf.ts(T)) == _expect(sc, spawn_view, sim.shown(T)), (ev, T)
    for t in (float(2.0 ** 24), 1e12, float("nan")):
        assert sc.mobj_states_at(t) == _expect(sc, spawn_view, sim.shown(mf.tics(t))), (ev, t)
    sc.mobj_event(0)                                                                    # what = 0 clears the list
    plain = mf.Sim(wad)
    for T in (0, 31, 200):
        assert sc.mobj_states_at(mf.ts(T)) == _expect(sc, spawn_view, plain.shown(T)), T
    sc.close()


def test_the_events_tell_the_cases_apart(wad):
    """(what the tables promise, read off the model: kill with death 0, explode with xdeath 0, targets that are not live)"""
    base = mf.Sim(wad)
    T = 60
    for what, moved, stays in ((mf.KILL, {2035, 3001, 46}, {3004, 34, 2014}), (mf.EXPLODE, {2035, 3001, 3004}, {34, 2014, 46})):
        sim = mf.Sim(wad, events=[(what, 30)])
        for t, a, b in zip(sim.types, sim.state_ids(T), base.state_ids(T)):
            if t in moved:
                assert a != b, (what, t)
            if t in stays or t in (48, 2028):
                assert a == b, (what, t)
    boom = mf.Sim(wad, events=[(mf.EXPLODE, 30)]).state_ids(T)
    dead = mf.Sim(wad, events=[(mf.KILL, 30)]).state_ids(T)
    assert all(a == b for t, a, b in zip(base.types, boom, dead) if t == 2035)          # xdeath 0: explode is kill
    assert 0 in dead                                                                    # an object has gone to state 0


def test_states_of_the_longest_tics(dg, wad, spawn_view):
    infos = [(3001, 28, 29, 0), (2035, 29, 0, 0)]
    for ev in ([], [(mf.KILL, 1000)]):
        sim = mf.Sim(wad, infos=infos, events=ev)
        sc = _scene(dg, wad, infos=infos, events=ev)
        for T in (0, 1, 999, 1000, 1001, 32766, 32767, 32768, 33766, 33767, 33768, 65533, 65534, 65535, 98300, 98301, 98302, 3 * 65534 + 5, 4000000):
            assert sc.mobj_states_at(mf.ts(T)) == _expect(sc, spawn_view, sim.shown(T)), (ev, T)
        assert sc.mobj_states_at(1e12) == _expect(sc, spawn_view, sim.shown(2 ** 32 - 1))
        sc.close()


def test_precedence_over_the_scene_state_and_flags_zero(dg, wad, spawn_view):
    sim = mf.Sim(wad)
    sc = _scene(dg, wad)
    driven = sim.driven.index(True)
    static = sim.driven.index(False)
    before = sc.sprite_frame("BAR1", 0), sc.sprite_frame("TROO", 3)
    sc.set_mobj_state(driven, None)                                                     # the thinker wins over the scene's state
    sc.set_mobj_state(static, "CAND", 1, True)                                          # an object it does not drive keeps the scene's
    want = _expect(sc, spawn_view, sim.shown(50))
    want[static] = (sc.sprite_frame("CAND", 1), 1)
    assert sc.mobj_states_at(mf.ts(50)) == want
    sc.set_mobj_thinkers(0)                                                             # off: the scene's states, the table dropped
    want = list(spawn_view)
    want[driven], want[static] = (-1, 0), (sc.sprite_frame("CAND", 1), 1)
    assert sc.mobj_states_at(mf.ts(50)) == want
    assert (sc.sprite_frame("BAR1", 0), sc.sprite_frame("TROO", 3)) == before           # ids never move
    sc.close()


def test_frames_of_live_chains_are_appended(dg, wad):
    a, b = dg.Scene(wad, "E1M1"), dg.Scene(wad, "E1M1")
    b.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    for d in mf.synth.SPRITE_DEFS:
        assert a.sprite_frame(d[1], 0) == b.sprite_frame(d[1], 0)                       # the frames of the spawn view kept their ids
    n0 = max(a.sprite_frame(s[1], 0) for s in mf.synth.SPRITE_DEFS)
    assert b.sprite_frame("TROO", 3) > n0 and b.sprite_frame("POSS", 2) > n0
    with pytest.raises(dg.DoomGpuError):
        b.sprite_frame("XXXX", 0)
    a.close()
    b.close()


def _records(fl):
    rs = [tuple(getattr(r, f) for f, _ in r._fields_) for r in fl.renders[:fl.n_renders]]
    cols = [tuple(getattr(c, f) for f, _ in c._fields_) for c in fl.columns[:fl.n_columns]]
    vps = [tuple(getattr(v, f) for f, _ in v._fields_) for v in fl.visplanes[:fl.n_visplanes]]
    return rs, cols, vps, list(fl.plane_tb[:fl.n_plane_tb]), [(o.kind, o.index) for o in fl.order[:fl.n_order]]


@pytest.mark.parametrize("ev", [[], EVENT_LISTS[7]])
def test_host_walker_equals_the_states_applied(dg, wad, path1993, ev):
    sim = mf.Sim(wad, events=ev)
    sc = _scene(dg, wad, events=ev)
    plain = dg.Scene(wad, "E1M1")
    plain.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)                   # (decodes the same frames in the same order, so that
    plain.set_mobj_thinkers(0)                                                          # the two scenes' bitmap ids can be compared)
    fresh = dg.Scene(wad, "E1M1")
    changed = 0
    for t in [0.0, 0.2, 0.5, 1.3, 2.75, 17.0, 123.4, 1e5, float(2.0 ** 24), float("inf"), float("nan"), -2.0]:
        for i, s in enumerate(sim.shown(mf.tics(t))):
            if s == "null":
                plain.set_mobj_state(i, None)
            elif s is not None:
                plain.set_mobj_state(i, s[0], s[1], bool(s[2]))
        views = dg.make_views(path1993[VIEWS], timestamp=t)
        for k in range(len(VIEWS)):
            got = _records(sc.build_lists(320, 200, views[k]))
            assert got == _records(plain.build_lists(320, 200, views[k])), (t, k)
            changed += got != _records(fresh.build_lists(320, 200, views[k]))
    assert changed >= 24                                                                # the states do reach these views
    for s in (sc, plain, fresh):
        s.close()


def test_flags_zero_lists_are_unchanged(dg, wad, path1993):
    a = dg.Scene(wad, "E1M1")
    b = dg.Scene(wad, "E1M1")
    b.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    b.mobj_event(mf.KILL, 1.0)
    b.set_mobj_thinkers(0)
    views = dg.make_views(path1993[VIEWS], timestamp=17.0)
    for k in range(len(VIEWS)):
        assert _records(a.build_lists(320, 200, views[k])) == _records(b.build_lists(320, 200, views[k])), k
    a.close()
    b.close()


def _tables(dg, states, infos):
    sa = (dg.DgStateRec * len(states))(*[dg.DgStateRec(s[0].encode(), s[1], s[2], s[3], s[4]) for s in states])
    ia = (dg.DgMobjInfoRec * max(1, len(infos)))(*[dg.DgMobjInfoRec(*r) for r in infos])
    return sa, ia


def test_error_returns(dg, wad):
    L = dg.lib()
    sc = dg.Scene(wad, "E1M1")
    sa, ia = _tables(dg, mf.STATES, mf.INFOS)
    ns, ni = len(mf.STATES), len(mf.INFOS)
    INV = dg.DG_ERR_INVALID
    for bad in (2, 3, 0x80000000, 0xFFFFFFFF):
        assert L.dg_scene_set_mobj_thinkers(sc._h, bad, sa, ns, ia, ni) == INV
    assert L.dg_scene_set_mobj_thinkers(None, 1, sa, ns, ia, ni) == INV
    assert L.dg_scene_set_mobj_thinkers(sc._h, 1, None, ns, ia, ni) == INV
    assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, ns, None, ni) == INV
    for bad_n in (0, -1, 65537):
        assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, bad_n, ia, ni) == INV
    assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, ns, ia, -1) == INV

    def with_state(i, **kw):
        rows = [list(s) for s in mf.STATES]
        for key, v in kw.items():
            rows[i][{"tics": 3, "next": 4}[key]] = v
        return _tables(dg, rows, mf.INFOS)[0]
    for i, kw in ((28, {"tics": -2}), (28, {"tics": -32768}), (5, {"next": ns}), (5, {"next": -1}), (0, {"next": 2 ** 31 - 1})):
        assert L.dg_scene_set_mobj_thinkers(sc._h, 1, with_state(i, **kw), ns, ia, ni) == INV, (i, kw)
    for col in (1, 2, 3):
        for v in (ns, -1):
            rows = [list(r) for r in mf.INFOS]
            rows[8][col] = v                                                            # (even in a row no thing uses)
            assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, ns, _tables(dg, mf.STATES, rows)[1], ni) == INV, (col, v)
    # events: only with the setting on, known kinds, never back in time, sixteen at most
    assert L.dg_scene_mobj_event(None, 1, 0.0) == INV
    assert L.dg_scene_mobj_event(sc._h, 1, 0.0) == INV                                  # nothing above was accepted: still off
    assert L.dg_scene_mobj_event(sc._h, 0, 0.0) == dg.DG_OK
    assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, ns, ia, ni) == dg.DG_OK
    for bad in (-1, 4, 255):
        assert L.dg_scene_mobj_event(sc._h, bad, 0.0) == INV
    assert L.dg_scene_mobj_event(sc._h, 1, 2.0) == dg.DG_OK
    assert L.dg_scene_mobj_event(sc._h, 2, 1.9) == INV
    assert L.dg_scene_mobj_event(sc._h, 2, 2.0) == dg.DG_OK                             # the same tics: allowed
    for _ in range(mf.MAX_EVENTS - 2):
        assert L.dg_scene_mobj_event(sc._h, 3, 5.0) == dg.DG_OK
    assert L.dg_scene_mobj_event(sc._h, 3, 5.0) == INV                                  # the 17th
    n = sc.mobj_count()
    buf = (dg.DgMobjState * (n + 1))()
    for bad_n in (n - 1, n + 1, 0, -1):
        assert L.dg_scene_mobj_states_at(sc._h, 1.0, buf, bad_n) == INV
    assert L.dg_scene_mobj_states_at(None, 1.0, buf, n) == INV
    assert L.dg_scene_mobj_states_at(sc._h, 1.0, None, n) == INV
    assert L.dg_scene_mobj_states_at(sc._h, 1.0, buf, n) == dg.DG_OK
    assert [buf[i].mobj for i in range(n)] == list(range(n))
    assert L.dg_scene_set_mobj_thinkers(sc._h, 0, None, 0, None, 0) == dg.DG_OK         # off: the tables are not read
    assert L.dg_scene_set_mobj_thinkers(sc._h, 1, sa, ns, None, 0) == dg.DG_OK          # no rows at all: nothing is driven
    assert sc.mobj_states_at(3.0) == sc.mobj_states_at(0.0)
    assert ctypes.sizeof(dg.DgStateRec) == 12 and ctypes.sizeof(dg.DgMobjInfoRec) == 16
    sc.close()


def test_a_new_table_drops_the_events(dg, wad, spawn_view):
    sc = _scene(dg, wad, events=[(mf.KILL, 3)])
    sc.set_mobj_thinkers(dg.DG_MOBJ_THINKERS, mf.STATES, mf.INFOS)
    assert sc.mobj_states_at(mf.ts(50)) == _expect(sc, spawn_view, mf.Sim(wad).shown(50))
    sc.close()


def test_mobj_rows_kernel_has_no_lds_and_no_scratch():
    from test_wall_fx_isa import _kernels
    ks = _kernels("mobj_fx_kernels.hip")
    hits = [(n, v) for n, v in ks.items() if "dg_mobj_rows" in n]
    assert len(hits) == 1, list(ks)
    name, (lds, scratch, vgpr) = hits[0]
    assert lds == 0 and scratch == 0 and vgpr <= 64, (name, lds, scratch, vgpr)


def test_mobj_rows_kernel_is_built_into_the_library(dg):
    mk = open(os.path.join(os.path.dirname(dg.LIB_PATH), "csrc", "Makefile")).read()
    assert "mobj_fx_kernels.hip" in mk
