"""mrt_render_views: many cameras of one scene in one wavefront render.

View v must be exactly set_camera(camera_v) + render(seed = seed_v): the
oracle's render of that camera and seed (bounces bit-exact, radiance within
the project's render tolerance), and the separate renders of the same context
bit for bit — through the refill (more work items than pool slots), through
chunks of the results slab, over shards, on a scene off the drain hand-off
path, and whatever the context's own camera is."""
import ctypes as C

import numpy as np
import pytest

import massrt
import oracle
from conftest import walk_keys

pytestmark = pytest.mark.gpu
ASPECT = float(massrt.ASPECT_RATIO)
RTOL = 1e-4  # relative L2 on accumulated radiance (README "Parity")
MRT_ERR_INVALID, MRT_ERR_STATE = 1, 4

# 21 x 13 is ragged against the 8 x 8 tiles, and W H spp = 819 work items per
# view is no multiple of 64: waves straddle two views
W, H, SPP_BEGIN, SPP = 21, 13, 2, 3
LOOK_AT = (0.0, 0.0, 0.0)
# (look_from, aperture, seed): three cameras, the second with a lens (its
# rejection draws shift the stream), the first again with another seed, the
# first again as it is
VIEWS = [((6.0, 8.0, 5.0), 0.0, 11), ((-7.0, 5.0, 4.0), 0.3, 12), ((2.0, 10.0, -6.0), 0.0, 13),
         ((6.0, 8.0, 5.0), 0.0, 14), ((6.0, 8.0, 5.0), 0.0, 11)]


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def camera(look_from, aperture=0.0):
    return massrt.make_camera(40.0, look_from, LOOK_AT, aspect=ASPECT, aperture=aperture)


def views_of(spec):
    return [massrt.MrtView(camera(f, ap), seed) for f, ap, seed in spec]


def one_by_one(c, views, w, h, spp_begin, spp, **kw):
    """The views as separate renders of context c: set_camera + render(seed)."""
    rgb = np.zeros((len(views), w * h * 3), np.float32)
    bo = np.zeros((len(views), w * h), np.uint32)
    for v, view in enumerate(views):
        c.set_camera(view.camera)
        c.render(w, h, spp_begin, spp, seed=view.seed, accum=(rgb[v], bo[v]), **kw)
    return rgb, bo


@pytest.fixture(scope="module")
def grid(golden_dir):
    return massrt.Builder(1).builtin("sphere_grid", ASPECT, golden_dir)


@pytest.fixture(scope="module")
def oracle_views(golden_dir):
    """The oracle's render of every view of VIEWS, once: (rgb [V, ..], bounces
    [V, ..], its counters summed over the views)."""
    o = oracle.Scene(1).builtin("sphere_grid", ASPECT, golden_dir)
    rgb, bo, total = [], [], {}
    for look_from, aperture, seed in VIEWS:
        o.camera(40.0, look_from, LOOK_AT, aspect=ASPECT, aperture=aperture)
        o.reset_counters()
        r, b = o.render(W, H, SPP_BEGIN, SPP, seed=seed)
        rgb.append(r)
        bo.append(b)
        for k, n in o.counters().items():
            total[k] = total.get(k, 0) + n
    return np.stack(rgb), np.stack(bo), total


def test_oracle_parity_per_view(ctx, grid, oracle_views):
    ctx.upload(grid)
    rgb, bo = ctx.render_views(W, H, views_of(VIEWS), SPP_BEGIN, SPP)
    orgb, obo, _ = oracle_views
    assert rgb.shape == (5, W * H * 3) and bo.shape == (5, W * H)
    for v in range(len(VIEWS)):
        assert np.array_equal(bo[v], obo[v]), f"view {v}: bounce counts differ from the oracle"
        assert rel_l2(rgb[v], orgb[v]) <= RTOL, v
    assert same_bits((rgb[4], bo[4]), (rgb[0], bo[0]))  # equal camera, equal seed
    assert not np.array_equal(bits(rgb[3]), bits(rgb[0]))  # equal camera, another seed
    assert obo.sum() > 0 and not np.array_equal(obo[1], obo[0]) and not np.array_equal(obo[2], obo[0])


def test_equals_separate_renders(ctx, grid):
    ctx.upload(grid)
    views = views_of(VIEWS)
    got = ctx.render_views(W, H, views, SPP_BEGIN, SPP)
    assert same_bits(got, one_by_one(ctx, views, W, H, SPP_BEGIN, SPP))
    # samples [0, 2) and then [2, 5) into the same arrays: one call for [0, 5)
    whole = ctx.render_views(W, H, views, 0, 5)
    rgb, bo = ctx.render_views(W, H, views, 0, 2)
    ctx.render_views(W, H, views, 2, 3, rgb=rgb, bounces=bo)
    assert same_bits((rgb, bo), whole)
    assert same_bits(whole, one_by_one(ctx, views, W, H, 0, 5))


# pool_paths 65536 is the smallest pool. The first case is 8 chunks of 2 spp
# (the slab of 2^14 samples against 6 x 960 list pixels; sample_base advances),
# each of 11,520 work items; the second is one chunk of 92,160 work items,
# more than the pool, so k_refill<ViewTable> generates the rest
@pytest.mark.parametrize("finish", [0, None], ids=["finish0", "finish_default"])
@pytest.mark.parametrize("results_log2", [14, None], ids=["chunks", "refill"])
def test_refill_chunks_shards(ctx, grid, results_log2, finish):
    w, h, spp = 40, 24, 16
    spec = [((6.0 - v, 8.0, 5.0 + 0.5 * v), 0.2 if v == 2 else 0.0, 100 + v) for v in range(6)]
    views = views_of(spec)
    walk = ctx.get_option("traversal")
    ref = massrt.Context(0, options={"traversal": walk})
    ref.upload(grid)
    want = one_by_one(ref, views, w, h, 0, spp)
    ref.close()
    opts = {"traversal": walk, "pool_paths": 65536}
    if results_log2 is not None:
        opts["results_log2"] = results_log2
    if finish is not None:
        opts["finish_paths"] = finish
    c = massrt.Context(0, options=opts)
    try:
        c.upload(grid)
        c.reset_kernel_stats()
        got = c.render_views(w, h, views, 0, spp, flags=massrt.RENDER_TIME_KERNELS)
        assert same_bits(got, want)
        if finish is None and results_log2 is None:
            assert c.kernel_stats()["finish_launches"] > 0  # the batch's one drain goes through the hand-off
        rgb = np.zeros_like(got[0])
        bo = np.zeros_like(got[1])
        for si in range(3):
            c.render_views(w, h, views, 0, spp, shard_index=si, shard_count=3, rgb=rgb, bounces=bo)
        assert same_bits((rgb, bo), want)
    finally:
        c.close()


def test_counters(ctx, grid, oracle_views):
    ctx.upload(grid)
    ctx.reset_counters()
    ctx.render_views(W, H, views_of(VIEWS), SPP_BEGIN, SPP, flags=massrt.RENDER_COUNTERS)
    gc, oc = ctx.counters(), oracle_views[2]
    assert gc["samples"] == len(VIEWS) * W * H * SPP
    for k in walk_keys(ctx, massrt.COUNTER_FIELDS):
        assert gc[k] == oc[k], (k, gc[k], oc[k])


def test_scene_off_the_handoff_path(ctx, golden_dir):
    """cornell_smoke: traversal draws (the fog boxes), the EXT k_shade, no drain hand-off."""
    b = massrt.Builder(1).builtin("cornell_smoke", ASPECT, golden_dir)
    ctx.upload(b)
    _, cam = b.desc()
    views = [massrt.MrtView(cam, 5),
             massrt.MrtView(massrt.make_camera(37.0, (6.0, 7.0, 18.0), (0.0, 5.0, 0.0), aspect=ASPECT), 6)]
    got = ctx.render_views(16, 9, views, 0, 2)
    assert same_bits(got, one_by_one(ctx, views, 16, 9, 0, 2))
    assert got[1].sum() > 0 and not np.array_equal(got[1][0], got[1][1])


def test_arguments_and_state(ctx, grid):
    L = massrt.lib()
    ctx.upload(grid)
    views = views_of(VIEWS[:2])
    arr = (massrt.MrtView * 2)(*views)
    rgb = np.zeros((2, W * H * 3), np.float32)
    bo = np.zeros((2, W * H), np.uint32)
    prgb, pbo = rgb.ctypes.data_as(C.POINTER(C.c_float)), bo.ctypes.data_as(C.POINTER(C.c_uint32))
    a = ctx.args(W, H, 0, 1, 0)
    for rc, text in ((L.mrt_render_views(ctx.h, C.byref(a), arr, 0, prgb, pbo), "no views"),
                     (L.mrt_render_views(ctx.h, C.byref(a), None, 2, prgb, pbo), "no views")):
        assert rc == MRT_ERR_INVALID and text in L.mrt_last_error(ctx.h).decode()
    fused = ctx.args(W, H, 0, 1, 0, flags=massrt.RENDER_FUSED)
    assert L.mrt_render_views(ctx.h, C.byref(fused), arr, 2, prgb, pbo) == MRT_ERR_INVALID
    assert "renders one camera" in L.mrt_last_error(ctx.h).decode()
    assert not rgb.any() and not bo.any()  # nothing was enqueued
    fresh = massrt.Context(0)
    assert L.mrt_render_views(fresh.h, C.byref(a), arr, 2, prgb, pbo) == MRT_ERR_STATE
    assert "no scene" in L.mrt_last_error(fresh.h).decode()
    fresh.close()


def test_context_camera_is_neither_needed_nor_changed(ctx, grid):
    views = views_of(VIEWS[:2])
    walk = ctx.get_option("traversal")
    c = massrt.Context(0, options={"traversal": walk})
    try:
        d, _ = grid.desc()
        c.upload_desc(d)  # a scene, no camera
        got = c.render_views(W, H, views, 0, 2)
        with pytest.raises(massrt.MassrtError, match="no camera"):
            c.render(W, H, 0, 2)
        a = c.args(W, H, 0, 2)
        assert massrt.lib().mrt_render(c.h, C.byref(a), got[0].ctypes.data_as(C.POINTER(C.c_float)),
                                       got[1].ctypes.data_as(C.POINTER(C.c_uint32))) == MRT_ERR_STATE
    finally:
        c.close()
    ctx.upload(grid)
    ctx.set_camera(camera(VIEWS[2][0]))
    before = ctx.render(W, H, 0, 2, seed=9)
    assert same_bits(ctx.render_views(W, H, views, 0, 2), got)
    assert same_bits(ctx.render(W, H, 0, 2, seed=9), before)


def test_simple_trace_gives_the_same_bits(ctx, grid):
    ctx.upload(grid)
    views = views_of(VIEWS[:3])
    assert same_bits(ctx.render_views(W, H, views, 0, 2, flags=massrt.RENDER_SIMPLE_TRACE),
                     ctx.render_views(W, H, views, 0, 2))
