"""The line-of-sight queries on the GPU (include/doomgpu.h: dg_sight_device, dg_sight_mobjs_device).  Every
device result is compared bit for bit with the host twin, which test_sight_host.py ties to np_sight's models.

  counts      dg_sight_queries with 1, 63, 64, 65 and 4097 queries over the families of the CPU tier, on the three worlds
  mobjs       dg_sight_mobjs with batches of 1, 3, 64 and 65 frames, on a map whose object count is no multiple of 32 and on the hand
              world's few objects, with and without poses and sector entries, and with entries in one frame of the batch alone
  capacity    a chain BSP exactly SIGHT_MAX_DEPTH deep gives the host twin's results; one node deeper both device calls return
              DG_ERR_CAPACITY with nothing launched, and the host twin still answers
  the rest    the same call twice, a scene switch, a colour slot left alone, the timing getter, a ctx without a scene
"""
import numpy as np
import pytest

import np_sight as ns
import sight_cases as sc
from test_sight_host import EYE, mobj_case

pytestmark = pytest.mark.gpu

MAX_BATCH = 65


@pytest.fixture(scope="module")
def scenes(dg):
    made = {}

    def get(world):
        if world not in made:
            made[world] = dg.Scene(sc.wad_of(world), "e1m1")
        return made[world]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def ctx(dg):
    c = dg.Context(64, 64, max_batch=MAX_BATCH, slots=1)
    yield c
    c.close()


def use(ctx, scene):
    if ctx._scene is not scene:
        ctx.upload_scene(scene)


def framed(q, n_frames):
    """The queries spread over n_frames frames."""
    q = q.copy()
    q["frame"] = np.arange(len(q)) % n_frames
    return q


# ---- counts ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,n", [("e1m1", 1), ("e1m1", 63), ("e1m1", 64), ("e1m1", 65), ("e1m1", 4097), ("holes", 4097), ("hand", 65), ("hand", 4097)])
def test_query_form_equals_the_host_twin(dg, ctx, scenes, world, n):
    scene = scenes(world)
    use(ctx, scene)
    q = sc.mixed(world, n)
    if n == 1:
        q = sc.families(world)["near"][:1].copy()
    want = dg.sight_host(scene, q)
    got = ctx.sight(q)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (world, n, np.flatnonzero(got != want)[:8].tolist())
    if n >= 63:
        assert 0 < want.sum() < n


def test_query_form_with_sector_entries_in_some_frames(dg, ctx, scenes):
    """Three frames, the door shut in frame 1 alone; then 4097 queries over MAX_BATCH frames with entries in one frame only."""
    scene, m = scenes("hand"), sc.model_of("hand")
    use(ctx, scene)
    pair, sector, shut = sc.hand_door()
    q = framed(np.repeat(pair, 3), 3)
    sa, keep = dg.make_view_sectors([[], [(sector, 24, 104), shut], []])
    assert ctx.sight(q, sa, 3).tolist() == [1, 0, 1] == dg.sight_host(scene, q, sa, 3).tolist()
    assert ctx.sight_kernel_ms()["rows_ms"] > 0
    assert ctx.sight(q, None, 3).tolist() == [1, 1, 1]
    big = framed(sc.mixed("hand", 4097), MAX_BATCH)
    entries = [[] for _ in range(MAX_BATCH)]
    entries[40] = [shut, (0, 8, 96)]
    sb, keep2 = dg.make_view_sectors(entries)
    want = dg.sight_host(scene, big, sb, MAX_BATCH)
    assert np.array_equal(ctx.sight(big, sb, MAX_BATCH), want)
    assert not np.array_equal(want, dg.sight_host(scene, big, None, MAX_BATCH))          # the entries decide some of them
    del keep, keep2


# ---- the mobjs form --------------------------------------------------------------------------------------------------------------------------

def batch_of(dg, world, n, with_poses, entries_kind):
    views1, poses1, entries1 = mobj_case(dg, world)
    k = len(views1)
    views = (dg.DgView * n)(*[views1[i % k] for i in range(n)])
    poses = [poses1[i % k] for i in range(n)] if with_poses else None
    if entries_kind == "all":
        entries = [entries1[i % k] for i in range(n)]
    elif entries_kind == "one":                                 # entries in one frame of the batch alone
        entries = [[] for _ in range(n)]
        entries[n // 2] = next(e for e in entries1 if e)
    else:
        entries = None
    return views, poses, entries


@pytest.mark.parametrize("world", ["holes", "hand"])
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_mobjs_form_equals_the_host_twin(dg, ctx, scenes, world, n):
    scene = scenes(world)
    use(ctx, scene)
    n_mobjs = scene.mobj_count()
    assert n_mobjs % 32 != 0
    heights = sc.mobj_heights(n_mobjs)
    for with_poses, entries_kind in ((False, None), (True, None), (False, "all"), (True, "all"), (True, "one"), (False, "one")):
        views, poses, entries = batch_of(dg, world, n, with_poses, entries_kind)
        pa, keep_p = dg.make_view_poses(poses) if poses is not None else (None, None)
        sa, keep_s = dg.make_view_sectors(entries) if entries is not None else (None, None)
        want = dg.sight_mobjs_host(scene, views, EYE, heights, pa, sa)
        got = ctx.sight_mobjs(views, EYE, heights, pa, sa)
        assert got.shape == want.shape == (n, (n_mobjs + 31) // 32) and np.array_equal(got, want), (world, n, with_poses, entries_kind)
        assert want.any() or n < 3, (world, n, with_poses, entries_kind)       # (a single viewer may see nothing)
        ms = ctx.sight_kernel_ms()
        has_rows = (with_poses and any(poses)) or (entries is not None and any(entries))
        assert ms["sight_ms"] > 0 and (ms["rows_ms"] > 0) == bool(has_rows), (ms, with_poses, entries_kind)
        del keep_p, keep_s


def test_mobjs_form_on_a_map_with_more_than_64_objects(dg, ctx, scenes, path1994):
    """More than one wavefront per frame: the heavy synthetic map's 300 objects, no multiple of 64, some of them moved."""
    scene = scenes("heavy")
    use(ctx, scene)
    n_mobjs = scene.mobj_count()
    assert n_mobjs > 64 and n_mobjs % 64 != 0 and n_mobjs % 32 != 0
    recs = path1994[[0, 250, 500, 750, 999]]
    views = dg.make_views(recs)
    heights = sc.mobj_heights(n_mobjs)
    poses = [[(m, float(recs[(f + 1) % 5][0]) + 4.0 * m, float(recs[(f + 1) % 5][1]), 0.0) for m in range(f, n_mobjs, 37)] for f in range(5)]
    pa, keep = dg.make_view_poses(poses)
    for p in (None, pa):
        want = dg.sight_mobjs_host(scene, views, EYE, heights, p)
        assert np.array_equal(ctx.sight_mobjs(views, EYE, heights, p), want) and want.any() and not (want[:, -1] >> np.uint32(n_mobjs % 32)).any()
    del keep


# ---- capacity --------------------------------------------------------------------------------------------------------------------------------

def test_a_bsp_at_the_capacity_runs_and_one_deeper_is_refused(dg, ctx, scenes):
    depth = sc.SIGHT_MAX_DEPTH
    at, over = scenes(f"chain{depth}"), scenes(f"chain{depth + 1}")
    assert at.bsp_depth() == depth and over.bsp_depth() == depth + 1
    use(ctx, at)
    q = sc.chain_queries(depth)
    want = dg.sight_host(at, q)
    assert np.array_equal(want, sc.model_of(f"chain{depth}").visible(q, sc.model_of(f"chain{depth}").height_rows(1))) and 0 < want.sum() < len(q)
    assert np.array_equal(ctx.sight(q), want)
    views = (dg.DgView * 2)(dg.DgView(8.0, 32.0, 0.0, 0.0, 0, 0, 0, 0, 0.0, 0), dg.DgView(64.0 * (depth + 1) - 8.0, 20.0, 0.0, 4.0, 0, 0, 0, 0, 0.0, 0))
    heights = np.full(at.mobj_count(), 56.0, dtype=np.float32)
    want_m = dg.sight_mobjs_host(at, views, EYE, heights)
    assert np.array_equal(ctx.sight_mobjs(views, EYE, heights), want_m) and want_m.any()
    before = ctx.sight_kernel_ms()
    use(ctx, over)
    q2 = sc.chain_queries(depth + 1)
    for call in (lambda: ctx.sight(q2), lambda: ctx.sight_mobjs(views, EYE, np.full(over.mobj_count(), 56.0, dtype=np.float32))):
        with pytest.raises(dg.DoomGpuError) as e:
            call()
        assert e.value.code == dg.DG_ERR_CAPACITY
    assert ctx.sight_kernel_ms() == before                       # nothing was launched
    m = sc.model_of(f"chain{depth + 1}")
    assert np.array_equal(dg.sight_host(over, q2), m.visible(q2, m.height_rows(1)))      # the host twin has no limit


# ---- the rest --------------------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_gives_the_same_bytes(dg, ctx, scenes):
    scene = scenes("e1m1")
    use(ctx, scene)
    q = sc.mixed("e1m1", 4097)
    assert np.array_equal(ctx.sight(q), ctx.sight(q))
    views, poses, entries = batch_of(dg, "holes", 3, True, "all")
    heights = sc.mobj_heights(scene.mobj_count())
    pa, keep_p = dg.make_view_poses(poses)
    sa, keep_s = dg.make_view_sectors(entries)
    assert np.array_equal(ctx.sight_mobjs(views, EYE, heights, pa, sa), ctx.sight_mobjs(views, EYE, heights, pa, sa))
    del keep_p, keep_s


def test_after_a_scene_switch_the_calls_use_the_new_scene(dg, ctx, scenes):
    q = sc.families("hand")["random"]
    a, b = scenes("hand"), scenes("e1m1")
    use(ctx, a)
    first = ctx.sight(q)
    use(ctx, b)
    second = ctx.sight(q)
    assert np.array_equal(first, dg.sight_host(a, q)) and np.array_equal(second, dg.sight_host(b, q)) and not np.array_equal(first, second)
    use(ctx, a)
    assert np.array_equal(ctx.sight(q), first)


def test_a_colour_slot_is_left_alone(dg, ctx, scenes, path1993):
    scene = scenes("e1m1")
    use(ctx, scene)
    ctx.submit(0, dg.make_views(path1993[[0, 297, 623]]))
    before = ctx.frame_checksums(0, 0, 3)
    ctx.sight(sc.mixed("e1m1", 65))
    views, poses, entries = batch_of(dg, "holes", 3, True, "all")
    pa, keep_p = dg.make_view_poses(poses)
    sa, keep_s = dg.make_view_sectors(entries)
    ctx.sight_mobjs(views, EYE, sc.mobj_heights(scene.mobj_count()), pa, sa)
    assert np.array_equal(ctx.frame_checksums(0, 0, 3), before)
    del keep_p, keep_s


def test_timing_and_a_ctx_without_a_scene(dg, ctx, scenes):
    fresh = dg.Context(64, 64, max_batch=4, slots=1)
    try:
        q = sc.families("hand")["near"]
        for call in (lambda: fresh.sight(q), fresh.sight_kernel_ms):
            with pytest.raises(dg.DoomGpuError) as e:
                call()
            assert e.value.code == dg.DG_ERR_INVALID
        fresh.upload_scene(scenes("hand"))
        with pytest.raises(dg.DoomGpuError) as e:
            fresh.sight(framed(sc.repeated(q, 8), 5), None, 5)                           # n_frames beyond max_batch
        assert e.value.code == dg.DG_ERR_CAPACITY
        assert np.array_equal(fresh.sight(q), dg.sight_host(scenes("hand"), q))
        ms = fresh.sight_kernel_ms()
        assert ms["sight_ms"] > 0 and ms["rows_ms"] == 0          # no frame had entries
        assert len(fresh.sight(q[:0])) == 0                       # n == 0 does nothing
    finally:
        fresh.close()
