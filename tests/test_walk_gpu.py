"""GPU tier of the player movement from recorded keys (dg_ctx_locate_walks).
1. The floors dg_ctx_locate_walks finds equal the host path's bit for bit, for calls of 1, 2 and 2^k - 1, 2^k, 2^k + 1 probes
   (k = 6 .. 21), many walks to a call (tests/walk_cases.py; the CPU tier checks that mix against the model).
2. Sixteen views of a walk located on the GPU, through all three front ends, equal the oracle's frames of the model's views.
3. A call while a slot is in flight leaves that slot's frames and the fallback counters as they are.
4. A walk of another scene, and a ctx with no scene uploaded: DG_ERR_INVALID.
5. A second call on located walks changes nothing and raises nothing.
6. Starts on the hand world's partition line, where a fused side test finds the other room: the host's and the model's floors."""
import ctypes

import numpy as np
import pytest

import walk_cases as wc
import walk_model as wm

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 320, 200
TURBO = 40                                                 # of the rendered walk


@pytest.fixture(scope="module")
def holes(dg, wad1993):
    wad = wc.holes_wad(wad1993)
    sc = dg.Scene(wad, "E1M1")
    yield sc, wm.Bsp(wad)
    sc.close()


@pytest.fixture(scope="module")
def calls(holes):
    return {total: descs for total, descs in wc.gpu_calls(holes[1])}


@pytest.fixture(scope="module")
def ctx(dg, holes):
    c = dg.Context(W, H, max_batch=16, slots=2, front_end=dg.DG_FE_HOST)
    c.upload_scene(holes[0])
    yield c
    c.close()


def _compare(dg, ctx, sc, descs, total):
    on_gpu = [dg.Walk(sc, k, start=s, turbo=t) for s, t, k in descs]
    on_host = [dg.Walk(sc, k, start=s, turbo=t) for s, t, k in descs]
    assert sum(w.probe_count() for w in on_gpu) == total
    ctx.locate_walks(on_gpu)
    for i, (g, h) in enumerate(zip(on_gpu, on_host)):
        a, b = g.floors().view(np.uint32), h.floors().view(np.uint32)
        assert np.array_equal(a, b), (total, i, len(a), np.flatnonzero(a != b)[:8])
    for w in on_gpu + on_host:
        w.close()


@pytest.mark.parametrize("k", [0] + list(range(6, 22)))
def test_gpu_floors_equal_host_floors(dg, ctx, holes, calls, k):
    for total in ([1, 2] if k == 0 else [(1 << k) - 1, 1 << k, (1 << k) + 1]):
        _compare(dg, ctx, holes[0], calls[total], total)


def test_starts_on_the_partition_line_of_the_hand_world(dg):
    """walk_cases.line_walks in one call: starts at which walk_left_of is 0.0 and a fused test is not (the import asserts that a fused
    model finds the other room's floor there), and exact ties.  The floors equal the host's and the model's; a library built with
    contraction on fails here."""
    wad = wc.hand_wad()
    sc, bsp = dg.Scene(wad, "E1M1"), wm.Bsp(wad)
    c = dg.Context(W, H, max_batch=1, slots=1)
    c.upload_scene(sc)
    descs = wc.line_walks()
    on_gpu = [dg.Walk(sc, k, start=s, turbo=t) for s, t, k in descs]
    on_host = [dg.Walk(sc, k, start=s, turbo=t) for s, t, k in descs]
    c.locate_walks(on_gpu)
    wrong = 0
    for (s, t, k), g, h in zip(descs, on_gpu, on_host):
        a, b, m = g.floors().view(np.uint32), h.floors().view(np.uint32), wm.walk(bsp, s, t, k).floors.view(np.uint32)
        wrong += not (np.array_equal(a, b) and np.array_equal(a, m))
    print(f"walks whose floors differ from the host's or the model's: {wrong} of {len(descs)}")
    assert wrong == 0
    for w in on_gpu + on_host:
        w.close()
    c.close()
    sc.close()


def test_sixteen_views_through_every_front_end_equal_the_oracle(dg, oracle, wad1993):
    sc = dg.Scene(wad1993, "E1M1")
    rng = np.random.default_rng(16)
    keys = rng.choice([wm.UP, wm.UP, wm.UP | wm.SHIFT, wm.LEFT, wm.RIGHT, wm.ALT | wm.LEFT, wm.UP | wm.LEFT, wm.DOWN], 600).astype(np.uint8)
    r = wm.walk(wm.Bsp(wad1993), None, TURBO, keys)
    times = [float(F(t)) for t in np.linspace(0.0, 17.0, 16)]
    want_views = wm.views(r, times)
    osc = oracle.Scene(wad1993, "e1m1")
    want = np.stack([np.frombuffer(osc.render(W, H, [float(v) for v in (m[0], m[1], m[2], m[4], m[5], m[6], m[7], m[3])] + [float(m[8])]),
                                   dtype=np.uint8).reshape(H, W, 3) for m in want_views])
    osc.close()
    # the inputs, by the model and the oracle alone: at this pace the walk stays inside the map (at turbo 100 it is outside, in front
    # of black frames, from the tenth view on), every view shows another frame, and the floor changes on the way
    assert len({want[i].tobytes() for i in range(16)}) == 16 and len(set(want_views[:, 3].tolist())) >= 2
    for fe in (dg.DG_FE_HOST, dg.DG_FE_DEVICE, dg.DG_FE_DEVICE_SEGS):
        c = dg.Context(W, H, max_batch=16, slots=1, front_end=fe)
        c.upload_scene(sc)
        w = dg.Walk(sc, keys, turbo=TURBO)
        c.locate_walks([w])
        out = c.render(w.views(times))
        bad = [i for i in range(16) if not np.array_equal(out[i], want[i])]
        assert not bad, (fe, bad)
        w.close()
        c.close()
    sc.close()


def test_slots_in_flight_are_left_alone(dg, wad1993, path1993):
    sc = dg.Scene(wad1993, "E1M1")
    views = dg.make_views(path1993[::63][:16])
    keys = np.full(5000, wm.UP | wm.ALT | wm.LEFT, dtype=np.uint8)
    for fe in (dg.DG_FE_DEVICE, dg.DG_FE_DEVICE_SEGS):
        c = dg.Context(W, H, max_batch=16, slots=2, front_end=fe)
        c.upload_scene(sc)
        c.submit(0, views)
        c.wait(0)
        want = c.readback(0, 0, 16)
        before = c.fallbacks()
        w = dg.Walk(sc, keys)
        c.submit(1, views)
        c.locate_walks([w])                                  # slot 1 is in flight
        c.wait(1)
        assert np.array_equal(c.readback(1, 0, 16), want), fe
        assert c.fallbacks() == before
        ref = dg.Walk(sc, keys)
        assert np.array_equal(w.floors().view(np.uint32), ref.floors().view(np.uint32))
        for q in (w, ref):
            q.close()
        c.close()
    sc.close()


def test_wrong_scene_and_no_scene(dg, wad1993, holes):
    lib = dg.lib()
    other = dg.Scene(wad1993, "E1M1")
    w_other = dg.Walk(other, [wm.UP] * 4)
    w_ok = dg.Walk(holes[0], [wm.UP] * 4)
    c = dg.Context(W, H, max_batch=1, slots=1)
    arr = (ctypes.c_void_p * 2)(w_ok._h, w_other._h)
    assert lib.dg_ctx_locate_walks(c._h, arr, 1) == dg.DG_ERR_INVALID             # no scene uploaded
    c.upload_scene(holes[0])
    assert lib.dg_ctx_locate_walks(c._h, arr, 2) == dg.DG_ERR_INVALID             # a walk of another scene
    assert lib.dg_ctx_locate_walks(c._h, None, 1) == dg.DG_ERR_INVALID
    assert lib.dg_ctx_locate_walks(c._h, (ctypes.c_void_p * 1)(None), 1) == dg.DG_ERR_INVALID
    assert lib.dg_ctx_locate_walks(c._h, arr, 1) == dg.DG_OK and lib.dg_ctx_locate_walks(c._h, None, 0) == dg.DG_OK
    ref = dg.Walk(holes[0], [wm.UP] * 4)
    assert np.array_equal(w_ok.floors().view(np.uint32), ref.floors().view(np.uint32))
    for w in (w_other, w_ok, ref):
        w.close()
    c.close()
    other.close()


def test_second_call_on_located_walks_changes_nothing(dg, ctx, holes, calls):
    sc = holes[0]
    walks = [dg.Walk(sc, k, start=s, turbo=t) for s, t, k in calls[1025]]
    ctx.locate_walks(walks + walks[:3])                      # a walk named twice is located once
    first = [w.floors().copy() for w in walks]
    ctx.locate_walks(walks)
    host = dg.Walk(sc, calls[65][1][2], start=calls[65][1][0], turbo=calls[65][1][1])
    host.floors()                                            # located on the host: skipped too
    ctx.locate_walks(walks + [host])
    for w, f in zip(walks, first):
        assert np.array_equal(w.floors().view(np.uint32), f.view(np.uint32))
    for w in walks + [host]:
        w.close()
