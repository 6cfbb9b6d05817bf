"""CPU tier of the player movement from recorded keys (dg_walk_*): dg_walk_views and dg_walk_floors equal the
model of tests/walk_model.py bit for bit, on the light map and on the vanilla-shaped one (seed 1995, oblique partitions), both with
subsectors emptied so that a position can be in no sector (tests/walk_cases.py says why that takes a doctored map).  Also: every
error return, dg_build_lists on a walk's view, the exported symbols, the new host code under ASan + UBSan, and the inputs of the
GPU tier's floor comparison checked against the conditions the contract sets for them, by the model alone."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import walk_cases as wc
import walk_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "doom-rust-renderer_amd", "csrc")
F = np.float32
L, R, U, D, A, S = wm.LEFT, wm.RIGHT, wm.UP, wm.DOWN, wm.ALT, wm.SHIFT
MAPS = ["light", "vanilla"]


@pytest.fixture(scope="module")
def maps(dg, wad1993, wad1995):
    """name -> (wad, product scene, model Bsp)"""
    out = {}
    for name, raw in (("light", wad1993), ("vanilla", wad1995)):
        wad = wc.holes_wad(raw)
        out[name] = (wad, dg.Scene(wad, "E1M1"), wm.Bsp(wad))
    yield out
    for _, sc, _ in out.values():
        sc.close()


def _bits(a):
    """The f32 bit patterns, every NaN as one pattern: IEEE 754 leaves a NaN's sign and payload to the implementation (libm's
    sinf(-inf) and a compiler's folding of it differ in the sign bit), so "bit for bit" is over numbers, infinities and zeros."""
    a = np.asarray(a, dtype=F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _edge_times(n):
    """Timestamps at, and one ulp below, tic boundaries; beyond the end; NaN; -0.0; negative — in no particular order."""
    ts = []
    for T in sorted({0, 1, 2, 3, max(n - 1, 0), n, n + 1, n + 7}):
        t = F(T) / F(35.0)
        while wm.tics_of(t) < T:                             # the smallest f32 whose tic count is T
            t = np.nextafter(t, F(np.inf))
        while T and wm.tics_of(np.nextafter(t, F(-np.inf))) >= T:
            t = np.nextafter(t, F(-np.inf))
        ts += [float(t), float(np.nextafter(t, F(-np.inf)))]
    ts += [1e9, float("inf"), float("nan"), -0.0, -1.0, float("-inf"), 5e-46]
    return [ts[i] for i in np.random.default_rng(n).permutation(len(ts))]


def _check(dg, sc, bsp, start, turbo, keys, times=None):
    """One walk against the model: floors, and views at `times` (default: the edge timestamps), bit for bit.  -> the model's result."""
    keys = np.asarray(keys, dtype=np.uint8)
    r = wm.walk(bsp, start, turbo, keys)
    w = dg.Walk(sc, keys, start=start, turbo=turbo)
    assert w.tics() == len(keys) and w.probe_count() == len(r.probes)
    times = _edge_times(len(keys)) if times is None else times
    got_v = w.views(times)                                   # views first: they locate on the host by themselves
    fl = w.floors()
    assert np.array_equal(_bits(fl), _bits(r.floors)), (start, turbo, np.flatnonzero(_bits(fl) != _bits(r.floors))[:4])
    want = wm.views(r, times)
    for i, ts in enumerate(times):
        v = got_v[i]
        got = [v.x, v.y, v.angle, v.floor_height, v.cos_a, v.sin_a, v.cos_na, v.sin_na, v.timestamp]
        assert np.array_equal(_bits(got), _bits(want[i, :9])), (start, turbo, ts, got, want[i])
        assert v.trig_valid == 1
    w.close()
    return r


def test_starts_on_the_partition_line_of_the_hand_world(dg):
    """walk_cases.line_walks: starts at which the side test is 0.0 and a fused one is not (room A's floor 0 against room B's 24), and exact
    ties on the partition, on segs and on vertices."""
    wad = wc.hand_wad()
    sc, bsp = dg.Scene(wad, "E1M1"), wm.Bsp(wad)
    floors = set()
    for start, turbo, keys in wc.line_walks():
        floors |= set(_check(dg, sc, bsp, start, turbo, keys, times=[0.0, 0.03, 1.0]).floors.tolist())
    assert floors == {0.0, 24.0}
    sc.close()


@pytest.mark.parametrize("name", MAPS)
def test_all_64_masks_held_for_three_tics(dg, maps, name):
    _, sc, bsp = maps[name]
    for k in range(64):
        _check(dg, sc, bsp, None, 100, [k] * 3)
        _check(dg, sc, bsp, (1000.5, 700.25, 2.5), 255, [k | (64 if k & 1 else 128)] * 3)      # bits 6 and 7 are ignored


@pytest.mark.parametrize("name", MAPS)
def test_opposite_keys_together(dg, maps, name):
    _, sc, bsp = maps[name]
    for keys in ([L | R] * 5, [A | L | R] * 5, [L | R | S, A | L | R | S, U | D, A | L | R | U | D | S] * 3):
        r = _check(dg, sc, bsp, (777.0, 1234.0, 1.0), 100, keys)
        assert len(r.probes) > 1 or not any(k & (A | U | D) for k in keys)


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("turbo", [0, 100, 255, -100, 32767])
def test_turbo(dg, maps, name, turbo):
    _, sc, bsp = maps[name]
    rng = np.random.default_rng(turbo & 0xFFFF)
    _check(dg, sc, bsp, None, turbo, rng.integers(0, 256, 120))


@pytest.mark.parametrize("name", MAPS)
def test_no_tics(dg, maps, name):
    _, sc, bsp = maps[name]
    r = _check(dg, sc, bsp, None, 100, [])
    assert len(r.floors) == 1
    _check(dg, sc, bsp, (wc.FAR, wc.FAR, 0.0), 100, [])


@pytest.mark.parametrize("name", MAPS)
def test_random_walks_and_any_f32_pose(dg, maps, name):
    _, sc, bsp = maps[name]
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        start = (float(F(rng.uniform(0, 4096))), float(F(rng.uniform(0, 3072))), float(F(rng.uniform(-7, 7))))
        _check(dg, sc, bsp, start, int(rng.choice([100, 255, 50])), rng.integers(0, 256, 700))
    for start in ((float("inf"), 0.0, 0.0), (100.0, float("nan"), 1.0), (3e38, -3e38, 1e30), (256.0, 256.0, float("inf"))):
        _check(dg, sc, bsp, start, 32767, [U, A | L, D | S, L, U] * 4, times=[0.0, 0.1, 0.3, 1.0])


@pytest.mark.parametrize("name", MAPS)
def test_far_outside_every_probe_misses(dg, maps, name):
    _, sc, bsp = maps[name]
    r = _check(dg, sc, bsp, (2048.0 + wc.FAR, 1536.0, 0.7), 100, [U, A | L | U, D | S, A | R] * 40)
    assert not r.hit.any() and not r.floors.any() and len(r.probes) > 160


@pytest.mark.parametrize("name", MAPS)
def test_leaves_the_map_and_comes_back(dg, maps, name):
    _, sc, bsp = maps[name]
    # 2 724 units a tic: out to the far ring in a dozen tics, and back again
    grid = [(float(x), float(y)) for y in range(300, 2900, 173) for x in range(300, 3900, 211)]
    inside = bsp.floor_at([g[0] for g in grid], [g[1] for g in grid])[0]
    x, y = grid[int(np.argmax(inside))]                      # the first grid point that lies in a sector
    r = _check(dg, sc, bsp, (x, y, 0.0), 32767, [U] * 14 + [D] * 14)
    hit = r.hit
    first_miss = int(np.argmin(hit))
    assert hit[0] and not hit[14] and hit[first_miss:].any(), hit                # the model shows it: out, and back in a sector
    assert r.floors[14] == r.floors[first_miss - 1]           # the floor sticks while the player is in no sector


def _sticky_walk(bsp):
    """A walk in which some tic's mid-tic probe hits and its last probe misses (searched once, seeds pinned by the loop order)."""
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        start = (float(F(rng.uniform(200, 3800))), float(F(rng.uniform(200, 2800))), float(F(rng.uniform(-3, 3))))
        keys = rng.choice([A | L | U, A | R | D, A | L | R | U | D, U | D | S, A | L | U | S, L, R], 400).astype(np.uint8)
        r = wm.walk(bsp, start, 255, keys)
        if r.sticky:
            return start, keys, r
    return None


@pytest.mark.parametrize("name", MAPS)
def test_mid_tic_hit_sticks_when_the_last_probe_misses(dg, maps, name):
    _, sc, bsp = maps[name]
    found = _sticky_walk(bsp)
    assert found is not None, "the model shows no such tic"
    start, keys, r = found
    t = r.sticky[0]
    lo, hi = r.end_of_tic[t - 1] + 1, r.end_of_tic[t]
    assert hi > lo and r.hit[lo:hi].any() and not r.hit[hi]                      # the model shows the case ...
    last_hit = lo + int(np.flatnonzero(r.hit[lo:hi])[-1])
    assert r.floors[t] == bsp.floor_at([r.probes[last_hit][0]], [r.probes[last_hit][1]])[1][0]
    _check(dg, sc, bsp, start, 255, keys)                                        # ... and the product agrees


def test_fast_model_equals_the_literal_model(maps):
    _, _, bsp = maps["light"]
    rng = np.random.default_rng(5)
    for n in (0, 1, 50, 3000):
        keys = wc._keys_for(rng, n)
        start = (float(F(rng.uniform(0, 4096))), float(F(rng.uniform(0, 3072))), float(F(rng.uniform(-3, 3))))
        r = wm.walk(bsp, start, 100, keys)
        xs, ys, end = wm.straight_probes(start, 100, keys)
        assert np.array_equal(_bits(xs), _bits([p[0] for p in r.probes])) and np.array_equal(_bits(ys), _bits([p[1] for p in r.probes]))
        assert list(end) == list(r.end_of_tic)
        assert np.array_equal(_bits(wm.floors_from_probes(bsp, xs, ys, end)[0]), _bits(r.floors))


def test_gpu_tier_inputs_meet_their_conditions(dg, maps):
    """The walks tests/test_walk_gpu.py locates, judged by the model alone: the totals, zero-tic walks, first probes that miss, walk
    boundaries on 2^k and 2^k +- 1, a run of misses beyond 2^13, 20 % .. 80 % misses overall and three floor heights or more.  The
    product's host path is compared on the way (every one of these 12.6 million probes)."""
    _, sc, bsp = maps["light"]
    calls = wc.gpu_calls(bsp)
    assert [t for t, _ in calls] == wc.TOTALS == [1, 2] + [(1 << k) + d for k in range(6, 22) for d in (-1, 0, 1)]
    probes = misses = zero_tic = first_miss = longest = 0
    heights, boundaries = set(), set()
    for total, descs in calls:
        at = 0
        for start, turbo, keys in descs:
            xs, ys, end = wm.straight_probes(start, turbo, keys)
            fl, hit = wm.floors_from_probes(bsp, xs, ys, end)
            w = dg.Walk(sc, keys, start=start, turbo=turbo)
            assert w.probe_count() == xs.size
            assert np.array_equal(_bits(w.floors()), _bits(fl)), (total, start, turbo)
            w.close()
            at += xs.size
            boundaries.add(at)
            misses += int(xs.size - hit.sum())
            zero_tic += keys.size == 0
            first_miss += not hit[0]
            heights |= set(fl[hit[end] | (fl != 0)].tolist())
            valid = hit.copy()
            valid[0] = True
            idx = np.flatnonzero(valid)
            longest = max(longest, int(np.diff(np.concatenate([idx, [valid.size]])).max()) - 1)
        assert at == total
        probes += total
    assert zero_tic >= 50 and first_miss >= 50
    assert all((1 << k) + d in boundaries for k in range(6, 21) for d in (-1, 0, 1))
    assert longest > 1 << 13
    assert 0.2 <= misses / probes <= 0.8, misses / probes
    assert len(heights) >= 3


def test_views_feed_build_lists_like_the_models(dg, wad1993):
    sc = dg.Scene(wad1993, "E1M1")                           # the map as it is: every frame can be built
    bsp = wm.Bsp(wad1993)
    rng = np.random.default_rng(3)
    keys = rng.choice([U, U, U | S, L, R, A | L, U | L, D], 300).astype(np.uint8)
    r = wm.walk(bsp, None, 100, keys)
    times = [float(F(t)) for t in np.linspace(0.0, 9.0, 12)]
    w = dg.Walk(sc, keys)
    got = w.views(times)
    want = wm.views(r, times)
    assert len({tuple(row[:3]) for row in want}) == len(times)                    # the views do move

    def records(fl):
        rs = [tuple(getattr(q, f) for f, _ in q._fields_) for q in fl.renders[:fl.n_renders]]
        cols = [tuple(getattr(c, f) for f, _ in c._fields_) for c in fl.columns[:fl.n_columns]]
        vps = [tuple(getattr(v, f) for f, _ in v._fields_) for v in fl.visplanes[:fl.n_visplanes]]
        return rs, cols, vps, list(fl.plane_tb[:fl.n_plane_tb]), [(o.kind, o.index) for o in fl.order[:fl.n_order]]

    for i in range(len(times)):
        m = want[i]
        mv = dg.DgView(*[float(v) for v in (m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8])], 1)
        assert records(sc.build_lists(320, 200, got[i])) == records(sc.build_lists(320, 200, mv)), i
    w.close()
    sc.close()


def test_error_returns(dg, maps, wad1993):
    lib = dg.lib()
    _, sc, _ = maps["light"]
    keys = (ctypes.c_uint8 * 8)(*[U] * 8)
    kp = ctypes.cast(keys, ctypes.POINTER(ctypes.c_uint8))
    h = ctypes.c_void_p()
    good = dg.DgWalkDesc(1.0, 2.0, 0.5, 0, 100, kp, 8)
    assert lib.dg_walk_create(None, ctypes.byref(good), ctypes.byref(h)) == dg.DG_ERR_INVALID
    assert lib.dg_walk_create(sc._h, None, ctypes.byref(h)) == dg.DG_ERR_INVALID
    assert lib.dg_walk_create(sc._h, ctypes.byref(good), None) == dg.DG_ERR_INVALID
    for bad in (dg.DgWalkDesc(1.0, 2.0, 0.5, 0, 100, None, 8),                   # keys == NULL with n_tics > 0
                dg.DgWalkDesc(1.0, 2.0, 0.5, 0, 100, kp, (1 << 22) + 1),         # n_tics above 1 << 22 (refused before keys are read)
                dg.DgWalkDesc(1.0, 2.0, 0.5, 0, 32768, kp, 8),                   # turbo outside i16
                dg.DgWalkDesc(1.0, 2.0, 0.5, 0, -32769, kp, 8)):
        assert lib.dg_walk_create(sc._h, ctypes.byref(bad), ctypes.byref(h)) == dg.DG_ERR_INVALID and not h.value
        assert lib.dg_last_error()
    assert lib.dg_walk_create(sc._h, ctypes.byref(dg.DgWalkDesc(0, 0, 0, 0, 100, None, 0)), ctypes.byref(h)) == dg.DG_OK   # no keys needed
    lib.dg_walk_free(h)
    # from_player_start on a map without a Player1Start: the same WAD with its type-1 things made type 2
    lump = wm._lumps(wad1993, "E1M1")["THINGS"]
    at = wad1993.index(lump)
    nostart = bytearray(wad1993)
    for i in range(len(lump) // 10):
        if struct.unpack_from("<h", lump, 10 * i + 6)[0] == 1:
            struct.pack_into("<h", nostart, at + 10 * i + 6, 2)
    s2 = dg.Scene(bytes(nostart), "E1M1")
    h = ctypes.c_void_p()
    assert lib.dg_walk_create(s2._h, ctypes.byref(dg.DgWalkDesc(0, 0, 0, 1, 100, kp, 8)), ctypes.byref(h)) == dg.DG_ERR_INVALID
    assert lib.dg_walk_create(s2._h, ctypes.byref(good), ctypes.byref(h)) == dg.DG_OK
    w = h
    buf = (ctypes.c_float * 16)()
    assert lib.dg_walk_tics(w) == 8 and lib.dg_walk_probe_count(w) == 9
    for n in (8, 10, 0, -1):
        assert lib.dg_walk_floors(w, buf, n) == dg.DG_ERR_INVALID
    assert lib.dg_walk_floors(None, buf, 9) == dg.DG_ERR_INVALID and lib.dg_walk_floors(w, None, 9) == dg.DG_ERR_INVALID
    assert lib.dg_walk_floors(w, buf, 9) == dg.DG_OK
    ts = (ctypes.c_float * 2)(0.0, 1.0)
    vs = (dg.DgView * 2)()
    assert lib.dg_walk_views(None, ts, 2, vs) == dg.DG_ERR_INVALID
    assert lib.dg_walk_views(w, None, 2, vs) == dg.DG_ERR_INVALID and lib.dg_walk_views(w, ts, 2, None) == dg.DG_ERR_INVALID
    assert lib.dg_walk_views(w, ts, -1, vs) == dg.DG_ERR_INVALID
    assert lib.dg_walk_views(w, ts, 2, vs) == dg.DG_OK and lib.dg_walk_views(w, None, 0, None) == dg.DG_OK
    assert lib.dg_walk_tics(None) == dg.DG_ERR_INVALID and lib.dg_walk_probe_count(None) == dg.DG_ERR_INVALID
    assert lib.dg_ctx_locate_walks(None, None, 0) == dg.DG_ERR_INVALID
    lib.dg_walk_free(w)
    lib.dg_walk_free(None)
    s2.close()


def test_header_symbols_are_exported_and_bound(dg):
    lib = dg.lib()
    names = ["dg_walk_create", "dg_walk_free", "dg_walk_tics", "dg_walk_probe_count", "dg_walk_floors", "dg_walk_views", "dg_ctx_locate_walks"]
    declared = dg.declared_symbols()
    for n in names:
        assert n in declared and hasattr(lib, n) and n in dg._SIGNATURES
    assert (dg.DG_KEY_LEFT, dg.DG_KEY_RIGHT, dg.DG_KEY_UP, dg.DG_KEY_DOWN, dg.DG_KEY_ALT, dg.DG_KEY_SHIFT) == (1, 2, 4, 8, 16, 32)
    assert ctypes.sizeof(dg.DgWalkDesc) == 40
    assert "ABI 4" in lib.dg_version().decode()


DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "walk.hpp"
using namespace dg;
int main(int argc, char **argv) {
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> wad((std::istreambuf_iterator<char>(f)), {});
    std::string err;
    Scene *sc = load_scene_from_wad(wad.data(), wad.size(), "E1M1", err);
    if (!sc) return 1;
    uint32_t s = 2463534242u;
    auto rnd = [&] { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    double sum = 0;
    const float inf = 1.0f / 0.0f;
    for (int i = 0; i < 300; i++) {
        std::vector<uint8_t> keys(i % 7 == 0 ? 0 : rnd() % 900);
        for (auto &k : keys) k = (uint8_t)rnd();
        dg_walk_desc d{(float)(rnd() % 8000) - 2000.0f, (float)(rnd() % 6000) - 1500.0f, (float)(rnd() % 700) / 100.0f, i % 3 == 0,
                       (int32_t)(rnd() % 65536) - 32768, keys.data(), (uint32_t)keys.size()};
        if (i % 50 == 1) d.x = inf;
        if (i % 50 == 2) d.angle = inf - inf;
        dg_walk *w = nullptr;
        if (walk_create(*sc, d, &w, err) != DG_OK) return 2;
        w->locate_host();
        if (w->floors.size() != keys.size() + 1 || w->end_of_tic.back() + 1 != w->px.size()) return 3;
        const float ts[] = {0.0f, -1.0f, inf - inf, 0.5f, 1e9f, inf, (float)keys.size() / 35.0f};
        for (float t : ts) { dg_view v; w->view_at(t, v); sum += v.floor_height; }
        delete w;
    }
    dg_walk_desc bad{0, 0, 0, 0, 100, nullptr, 5};
    dg_walk *w = nullptr;
    if (walk_create(*sc, bad, &w, err) != DG_ERR_INVALID || w) return 4;
    delete sc;
    std::printf("WALK SANITIZER DRIVER OK %g\n", sum);
    return 0;
}
"""


def test_walk_host_code_is_clean_under_asan_ubsan(tmp_path, maps):
    """The sanitizer tier's way (tests/test_sanitizers.py): a CPU build of the host sources with ASan + UBSan, here walk.cpp over
    random key streams, hostile poses and timestamps."""
    src = tmp_path / "walk_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "walk_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC, "-o", str(exe), str(src)] +
                          [os.path.join(CSRC, f) for f in ("walk.cpp", "scene.cpp", "frontend.cpp")])
    wad = tmp_path / "holes.wad"
    wad.write_bytes(maps["light"][0])
    r = subprocess.run([str(exe), str(wad)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and "WALK SANITIZER DRIVER OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
