"""mrt_render_adaptive on the GPU: every 8x8 tile sampled in rounds until its
error is met or the cap is spent.

The device's result must equal the numpy float32 restatement of the contract
(tests/adaptive_ref.py) run over the device's own 1-spp frames, bit for bit in
every buffer and in the report; a pixel that stopped after c samples must hold
the uniform c-spp render's bits and the oracle's bounce count; shards, chunked
results slabs and a render continued in a second call must change nothing; the
compaction must hold over many workgroups; the decision kernel must agree with
the host's on crafted and random moments; the resolve must display as the
uniform frames do. Each case runs on both walks (the `ctx` fixture)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import massrt
import oracle

pytestmark = pytest.mark.gpu
ASPECT = float(massrt.ASPECT_RATIO)
MRT_OK, MRT_ERR_INVALID, MRT_ERR_STATE = 0, 1, 4
W, H, SEED = 50, 27, 1  # ragged against the tiles: 7 x 4 of them, the right column 2 wide, the top row 3 high
RULE = dict(min_spp=8, step_spp=8, threshold=0.2, floor=0.01)
CAP = 96
KEYS = ("rgb", "bounces", "moments", "samples")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device_run(c, w, h, cap, spp_begin=0, accum=None, seed=SEED, **kw):
    rgb, bo, mom, smp, rep = c.render_adaptive(w, h, spp_begin, cap, seed=seed, accum=accum, **kw)
    assert c.debug_status() == [0, 0, 0, 0]  # the bounds-checked build recorded no bad index (MASSRT_LIB=dbg)
    return {"rgb": rgb, "bounces": bo, "moments": mom, "samples": smp, "report": rep}


def assert_same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, int((bits(got[k]) != bits(want[k])).sum()))
    if "report" in want and "report" in got:
        assert got["report"] == want["report"], what


_frames = {}


def device_frames(c, key, w, h, n, first=0, seed=SEED):
    """The context's own 1-spp frames of samples [first, first + n) of the scene
    it holds (`key` names it): what the restatement runs over. Once per walk."""
    k = (id(c), key, w, h, first, n, seed)
    if k not in _frames:
        fr = [c.render(w, h, first + s, 1, seed=seed) for s in range(n)]
        _frames[k] = ([f[0] for f in fr], [f[1] for f in fr])
    return _frames[k]


@pytest.fixture(scope="module")
def grid(golden_dir):
    return massrt.Builder(1).builtin("sphere_grid", W / H, golden_dir)  # the camera of the frame's own shape


@pytest.fixture(scope="module")
def grid_oracle(golden_dir):
    return oracle.Scene(1).builtin("sphere_grid", W / H, golden_dir)


def test_main_case(ctx, grid, grid_oracle):
    """sphere_grid 50x27, min 8, step 8, cap 96, threshold 0.2, floor 0.01."""
    ctx.upload(grid)
    rgb, bo = device_frames(ctx, "grid", W, H, CAP)
    want = adaptive_ref.run(W, H, rgb, bo, cap=CAP, **RULE)
    got = device_run(ctx, W, H, CAP, **RULE)
    print("open tiles after each round:", want["open"], "report:", got["report"])
    assert_same(got, want, "device vs restatement")
    counts = adaptive_ref.per_tile_counts(W, H, got["samples"])
    adaptive_ref.check_not_vacuous(counts, 8, CAP)
    assert got["report"]["samples"] == int(got["samples"].sum())
    for c in np.unique(counts):
        px = np.flatnonzero(got["samples"] == c)
        u_rgb, u_b = ctx.render(W, H, 0, int(c), seed=SEED)
        assert np.array_equal(bits(got["rgb"]).reshape(-1, 3)[px], bits(u_rgb).reshape(-1, 3)[px]), c
        assert np.array_equal(got["bounces"][px], u_b[px]), c
        _, o_b = grid_oracle.render_pixels(W, H, px, 0, int(c), seed=SEED)
        assert np.array_equal(got["bounces"][px], o_b), c


def test_min_equal_to_cap_is_the_uniform_render(ctx, grid):
    ctx.upload(grid)
    got = device_run(ctx, W, H, 12, min_spp=12, step_spp=5, threshold=0.2, floor=0.01)
    u_rgb, u_b = ctx.render(W, H, 0, 12, seed=SEED)
    assert np.array_equal(bits(got["rgb"]), bits(u_rgb)) and np.array_equal(got["bounces"], u_b)
    assert np.all(got["samples"] == 12)
    rep = got["report"]
    assert (rep["rounds"], rep["spp_reached"], rep["tiles"], rep["samples"]) == (1, 12, 28, 12 * W * H)


def test_huge_threshold_stops_at_the_minimum(ctx, grid):
    ctx.upload(grid)
    got = device_run(ctx, W, H, 64, min_spp=6, step_spp=8, threshold=1e6, floor=0.01)
    assert np.all(got["samples"] == 6)
    assert got["report"] == {"rounds": 1, "spp_reached": 6, "tiles": 28, "tiles_open": 0, "samples": 6 * W * H}
    u_rgb, u_b = ctx.render(W, H, 0, 6, seed=SEED)
    assert np.array_equal(bits(got["rgb"]), bits(u_rgb)) and np.array_equal(got["bounces"], u_b)


SMALL = dict(min_spp=4, step_spp=4, threshold=0.3, floor=0.01)


def test_shards_into_shared_buffers_equal_one_call(ctx, grid):
    ctx.upload(grid)
    whole = device_run(ctx, W, H, 24, **SMALL)
    assert len(np.unique(whole["samples"])) >= 3  # the shards' tiles stop at different times
    acc = (np.zeros(W * H * 3, np.float32), np.zeros(W * H, np.uint32), np.zeros(W * H * 2, np.float32),
           np.zeros(W * H, np.uint32))
    reps = [device_run(ctx, W, H, 24, accum=acc, shard_index=i, shard_count=3, **SMALL)["report"] for i in range(3)]
    assert_same(dict(zip(KEYS, acc)), {k: whole[k] for k in KEYS}, "3 shards")
    assert sum(r["samples"] for r in reps) == whole["report"]["samples"]
    assert [r["tiles"] for r in reps] == [10, 9, 9]
    assert sum(r["tiles_open"] for r in reps) == whole["report"]["tiles_open"]
    assert max(r["rounds"] for r in reps) == whole["report"]["rounds"]


def test_chunked_results_slab_changes_nothing(ctx, grid):
    ctx.upload(grid)
    whole = device_run(ctx, W, H, 24, **SMALL)
    c = massrt.Context(0, options={"traversal": ctx.tuning()["traversal"], "results_log2": 11})
    try:
        c.upload(grid)
        assert c.tuning()["results_max"] == 2048 and W * H < 2048 < 2 * W * H  # chunks of one sample per pixel
        assert_same(device_run(c, W, H, 24, **SMALL), whole, "results_log2 11")
    finally:
        c.close()


def test_continued_in_a_second_call(ctx, grid):
    ctx.upload(grid)
    whole = device_run(ctx, W, H, 32, **SMALL)
    first = device_run(ctx, W, H, 16, **SMALL)
    acc = tuple(first[k] for k in KEYS)
    second = device_run(ctx, W, H, 16, spp_begin=16, accum=acc, min_spp=0, step_spp=4, threshold=0.3, floor=0.01)
    assert_same(second, {k: whole[k] for k in KEYS}, "16 + 16 vs 32")
    assert first["report"]["samples"] + second["report"]["samples"] == whole["report"]["samples"]
    assert second["report"]["tiles_open"] == whole["report"]["tiles_open"]
    assert 16 < whole["samples"].max() and whole["samples"].min() < 16  # both calls decided something


def test_compaction_across_waves_and_workgroups(ctx, grid):
    """200 x 120: 375 tiles, two scan workgroups, 94 compaction workgroups."""
    w, h, cap = 200, 120, 16
    ctx.upload(grid)
    rgb, bo = device_frames(ctx, "grid", w, h, cap)
    want = adaptive_ref.run(w, h, rgb, bo, cap=cap, **SMALL)
    got = device_run(ctx, w, h, cap, **SMALL)
    assert_same(got, want, "200x120")
    assert want["report"]["tiles"] == 375 and 0 < want["open"][0] < 375 and len(set(want["open"])) >= 3, want["open"]
    # open and closed tiles alternate within waves' worth of tiles: the list is a real compaction
    still = adaptive_ref.per_tile_counts(w, h, got["samples"]) > 4
    assert 20 < int(np.abs(np.diff(still.astype(int))).sum())


@pytest.mark.parametrize("size", [(50, 27), (200, 120)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiles_device_agrees_with_the_host(ctx, size):
    import torch

    w, h = size
    dev = torch.device("cuda", 0)
    for si, sc in ((0, 1), (1, 3)):
        nt = massrt.adaptive_tile_count(w, h, si, sc)
        for name, mom, n, thr, fl in adaptive_ref.decision_cases(w, h):
            want = massrt.adaptive_tiles(w, h, mom, n, si, sc, threshold=thr, floor=fl)
            assert np.array_equal(want, adaptive_ref.tiles_open(w, h, mom, n, thr, fl, si, sc)), name
            d_mom = torch.from_numpy(np.ascontiguousarray(mom)).to(dev)
            d_n = torch.from_numpy(n.view(np.int32)).to(dev)
            d_open = torch.full((nt + 8,), 7, dtype=torch.uint8, device=dev)
            d_cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.adaptive_tiles_device(w, h, d_mom.data_ptr(), d_n.data_ptr(), d_open.data_ptr(), d_cnt.data_ptr(), si,
                                      sc, threshold=thr, floor=fl)
            torch.cuda.synchronize()
            out = d_open.cpu().numpy()
            assert np.array_equal(out[:nt], want), (name, si, sc)
            assert np.all(out[nt:] == 7) and int(d_cnt.cpu()[0]) == int(want.sum()), (name, si, sc)


def test_resolve_and_display(ctx, grid):
    ctx.upload(grid)
    got = device_run(ctx, W, H, 24, **SMALL)
    res = ctx.adaptive_resolve(W, H, got["rgb"], got["samples"])
    assert np.array_equal(bits(res), bits(adaptive_ref.resolve(got["rgb"], got["samples"])))
    shown = ctx.tonemap(W, H, res, got["bounces"], 1)
    counts = np.unique(got["samples"])
    assert len(counts) >= 3
    for c in counts:
        u_rgb, u_b = ctx.render(W, H, 0, int(c), seed=SEED)
        uniform = ctx.tonemap(W, H, u_rgb, u_b, int(c))
        here = (got["samples"] == c).reshape(H, W)[::-1]  # the bytes are top row first
        assert np.array_equal(shown[here], uniform[here]), c
    # pixels without samples resolve to zeros, whatever the sums hold
    n = got["samples"].copy()
    n[::7] = 0
    res0 = ctx.adaptive_resolve(W, H, got["rgb"], n)
    assert np.array_equal(bits(res0), bits(adaptive_ref.resolve(got["rgb"], n))) and np.all(res0.reshape(-1, 3)[::7] == 0)
    # the sample map through the Depth view: count / max count
    depth = ctx.tonemap(W, H, res, got["samples"], 1, massrt.DISPLAY_DEPTH)
    assert depth.shape == (H, W, 3) and len(np.unique(depth[..., 0])) == len(counts)
    assert np.all(depth[(got["samples"] == counts[-1]).reshape(H, W)[::-1]] == 255)


def _raw(c, args, p, rgb, bo, mom, smp):
    f32, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return massrt.lib().mrt_render_adaptive(c.h, None if args is None else C.byref(args), None if p is None else C.byref(p),
                                            ptr(rgb, f32), ptr(bo, u32), ptr(mom, f32), ptr(smp, u32), None)


def test_errors_and_no_ops(ctx, grid):
    ctx.upload(grid)
    n = W * H
    bufs = [np.zeros(n * 3, np.float32), np.zeros(n, np.uint32), np.zeros(n * 2, np.float32), np.zeros(n, np.uint32)]
    args = ctx.args(W, H, 0, 16, SEED)
    ok = massrt.adaptive_params(**SMALL)
    for k in range(4):
        b = list(bufs)
        b[k] = None
        assert _raw(ctx, args, ok, *b) == MRT_ERR_INVALID, k
    assert _raw(ctx, args, None, *bufs) == MRT_ERR_INVALID and _raw(ctx, None, ok, *bufs) == MRT_ERR_INVALID
    bad = [dict(min_spp=17), dict(step_spp=0), dict(threshold=-1.0), dict(threshold=float("nan")),
           dict(floor=float("inf")), dict(floor=-0.5)]
    for kw in bad:
        assert _raw(ctx, args, massrt.adaptive_params(**{**SMALL, **kw}), *bufs) == MRT_ERR_INVALID, kw
    assert _raw(ctx, ctx.args(W, H, 0, 4097, SEED), massrt.adaptive_params(min_spp=0, step_spp=1), *bufs) == MRT_ERR_INVALID
    for flags in (massrt.RENDER_FUSED, massrt.RENDER_SIMPLE_TRACE):
        assert _raw(ctx, ctx.args(W, H, 0, 16, SEED, flags=flags), ok, *bufs) == MRT_ERR_INVALID, flags
    assert _raw(ctx, ctx.args(W, H, 2 ** 32 - 8, 16, SEED), ok, *bufs) == MRT_ERR_INVALID
    assert _raw(ctx, ctx.args(W, H, 0, 16, SEED, shard_index=2, shard_count=2), ok, *bufs) == MRT_ERR_INVALID
    assert all(not b.any() for b in bufs)  # nothing was enqueued
    # nothing to add: no depth, no samples
    for a in (ctx.args(W, H, 0, 16, SEED, max_depth=0), ctx.args(W, H, 0, 0, SEED)):
        assert _raw(ctx, a, massrt.adaptive_params(min_spp=0, step_spp=4), *bufs) == MRT_OK
        assert all(not b.any() for b in bufs)
    # the flags of a frame work as for a frame
    ctx.reset_counters()
    got = device_run(ctx, W, H, 8, flags=massrt.RENDER_COUNTERS | massrt.RENDER_TIME_KERNELS, **SMALL)
    assert ctx.counters()["samples"] == got["report"]["samples"] == int(got["samples"].sum())
    assert ctx.kernel_stats()["iterations"] > 0
    plain = device_run(ctx, W, H, 8, **SMALL)
    assert_same(got, plain, "counting render")


def test_state_error_before_upload():
    c = massrt.Context(0)
    try:
        n = W * H
        bufs = [np.zeros(n * 3, np.float32), np.zeros(n, np.uint32), np.zeros(n * 2, np.float32), np.zeros(n, np.uint32)]
        assert _raw(c, c.args(W, H, 0, 16, SEED), massrt.adaptive_params(**SMALL), *bufs) == MRT_ERR_STATE
    finally:
        c.close()


@pytest.fixture(scope="module")
def other_scenes(golden_dir):
    from conftest import REPO
    from gen_assets import ensure_assets

    eve_assets = ensure_assets(REPO / "assets", mesh=False, eve=True)
    return {"cornell_smoke": massrt.Builder(1).builtin("cornell_smoke", ASPECT, golden_dir),
            "eve": massrt.Builder(1).builtin("eve", ASPECT, eve_assets)}


@pytest.mark.parametrize("name", ["cornell_smoke", "eve"])
def test_scenes_with_traversal_draws_and_the_ext_variant(ctx, other_scenes, name):
    """cornell_smoke draws during the traversal (no drain hand-off); eve shades with the EXT variant."""
    w, h, cap = 48, 27, 12
    rule = dict(min_spp=4, step_spp=4, threshold=0.25, floor=0.01)
    ctx.upload(other_scenes[name])
    rgb, bo = device_frames(ctx, name, w, h, cap)
    want = adaptive_ref.run(w, h, rgb, bo, cap=cap, **rule)
    got = device_run(ctx, w, h, cap, **rule)
    print(name, "open tiles after each round:", want["open"])
    assert_same(got, want, name)
    assert want["report"]["rounds"] == 3 and want["open"][0] > 0, want["open"]  # some tiles sample to the cap
