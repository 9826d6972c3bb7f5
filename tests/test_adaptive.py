"""mrt_render_adaptive without a GPU: the tile decision (mrt_adaptive_tiles,
host only) against the numpy float32 restatement (tests/adaptive_ref.py) bit
for bit, the round schedule and the argument checks the library's host loop
runs (csrc/host/adaptive.h through tools/adaptive_check.cpp), and the whole
rule over the oracle's per-sample frames, where it must be seen to spread its
samples. On the GPU whole renders see them (tests/test_gpu_adaptive.py)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref
import massrt
import oracle
from conftest import REPO

MRT_OK, MRT_ERR_INVALID = 0, 1
SIZES = [(50, 27), (8, 8), (1, 1), (9, 17)]
SHARDS = [(0, 1), (0, 3), (1, 3), (2, 3), (0, 4), (3, 4)]


def test_defaults_and_struct_layouts(tmp_path):
    assert massrt.adaptive_defaults() == {"min_spp": 16, "step_spp": 128, "threshold": pytest.approx(0.05),
                                          "floor": pytest.approx(0.01)}
    assert massrt.lib().mrt_adaptive_default_params(None) == MRT_ERR_INVALID
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    structs = {"mrt_adaptive_params": massrt.MrtAdaptiveParams, "mrt_adaptive_report": massrt.MrtAdaptiveReport}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{REPO}/include/massrt.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    out = subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        key, val = line.rsplit(" ", 1)
        if key.endswith(" size"):
            assert C.sizeof(structs[key[:-5]]) == int(val), key
        else:
            cname, f = key.split(".")
            assert getattr(structs[cname], f).offset == int(val), key


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decision_equals_the_restatement(size):
    W, H = size
    seen = set()
    for name, mom, n, thr, fl in adaptive_ref.decision_cases(W, H):
        for si, sc in SHARDS:
            want = adaptive_ref.tiles_open(W, H, mom, n, thr, fl, si, sc)
            got = massrt.adaptive_tiles(W, H, mom, n, si, sc, threshold=thr, floor=fl)
            assert got.shape == want.shape == (massrt.adaptive_tile_count(W, H, si, sc),), (name, si, sc)
            assert np.array_equal(got, want), (name, si, sc, got, want)
        seen.add((name, tuple(adaptive_ref.tiles_open(W, H, mom, n, thr, fl).tolist())))
    verdict = dict(seen)
    # what the crafted cases are for, on the restatement alone
    assert not any(verdict["calm"]) and not any(verdict["zero variance"]) and not any(verdict["calm, floor 0"])
    assert not any(verdict["zero variance, threshold 0"]) and all(verdict["calm, threshold 0"])
    assert not any(verdict["L slightly negative"]) and not any(verdict["L slightly negative, threshold 0"])
    for name in ("n 0 in one slot", "n 1 in one slot", "m1 nan", "m2 nan", "m2 +inf", "a noisy pixel"):
        v = verdict[name]  # the changed pixels' tiles, the first and the last, are open; the rest closed
        assert v[0] == 1 and v[-1] == 1 and sum(v) == min(2, len(v)), (name, v)
    # -inf is no NaN: L = -inf compares below any R (an infinite m1 gives L = -inf, R = +inf)
    for name in ("n 2 in one slot", "m2 -inf", "m1 +inf", "m1 -inf"):
        assert not any(verdict[name]), name
    if W * H > 1000:  # 28 tiles
        v = verdict["random thr 0.2 floor 0.01"]
        assert 0 < sum(v) < len(v), v  # both outcomes


def test_decision_on_many_random_tiles():
    W, H = 200, 120
    mom, n = adaptive_ref.random_moments(W, H, 9)
    for thr, fl in ((0.2, 0.01), (0.02, 0.0), (0.7, 0.3)):
        want = adaptive_ref.tiles_open(W, H, mom, n, thr, fl)
        got = massrt.adaptive_tiles(W, H, mom, n, threshold=thr, floor=fl)
        assert np.array_equal(got, want), (thr, fl)
    want = adaptive_ref.tiles_open(W, H, mom, n, 0.2, 0.01)
    assert 0.1 < want.mean() < 0.9, want.mean()


def _tiles(W, H, si, sc, mom, n, p, open_, n_open):
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    return massrt.lib().mrt_adaptive_tiles(W, H, si, sc, None if mom is None else mom.ctypes.data_as(C.POINTER(C.c_float)),
                                           None if n is None else n.ctypes.data_as(u32),
                                           None if p is None else C.byref(p),
                                           None if open_ is None else open_.ctypes.data_as(u8), n_open)


def test_decision_argument_errors():
    W, H = 9, 17
    mom, n = np.zeros(W * H * 2, np.float32), np.zeros(W * H, np.uint32)
    out = np.zeros(6, np.uint8)
    ok = massrt.adaptive_params(threshold=0.2, floor=0.01)
    assert _tiles(W, H, 0, 1, mom, n, ok, out, None) == MRT_OK  # n_open is optional
    assert out.tolist() == [1] * 6  # no samples: everything open
    assert _tiles(W, H, 0, 1, mom, n, None, out, None) == MRT_ERR_INVALID
    assert _tiles(W, H, 0, 1, None, n, ok, out, None) == MRT_ERR_INVALID
    assert _tiles(W, H, 0, 1, mom, None, ok, out, None) == MRT_ERR_INVALID
    assert _tiles(W, H, 0, 1, mom, n, ok, None, None) == MRT_ERR_INVALID
    assert _tiles(0, H, 0, 1, mom, n, ok, out, None) == MRT_ERR_INVALID
    assert _tiles(W, H, 2, 2, mom, n, ok, out, None) == MRT_ERR_INVALID
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert _tiles(W, H, 0, 1, mom, n, massrt.adaptive_params(threshold=bad), out, None) == MRT_ERR_INVALID, bad
        assert _tiles(W, H, 0, 1, mom, n, massrt.adaptive_params(floor=bad), out, None) == MRT_ERR_INVALID, bad
    assert "threshold" in massrt.lib().mrt_global_last_error().decode() or "floor" in \
        massrt.lib().mrt_global_last_error().decode()
    with pytest.raises(TypeError, match="unknown adaptive parameter"):
        massrt.adaptive_params(treshold=0.1)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path_factory.mktemp("adaptive") / "adaptive_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(REPO / "tools" / "adaptive_check.cpp")], check=True)

    def run(*args):
        r = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
        return [ln.split(None, 1) for ln in r.stdout.splitlines()]

    return run


@pytest.mark.parametrize("rule", [(8, 8, 96), (16, 16, 1024), (4, 4, 16), (8, 8, 20), (5, 7, 40), (0, 16, 16),
                                  (0, 5, 12), (12, 3, 12), (0, 1, 0), (1, 1, 4096), (3, 1000, 10)])
def test_round_schedule(check, rule):
    mn, step, cap = rule
    out = check("rounds", mn, step, cap)
    got = [tuple(int(x) for x in rest.split()) for key, rest in out if key == "round"]
    want = adaptive_ref.schedule(mn, step, cap)
    assert got == [(r, first, count) for r, (first, count) in enumerate(want)]
    # by hand: round 0 the minimum, then steps from where the last round ended, ending exactly at the cap
    assert got[0] == (0, 0, mn) and sum(g[2] for g in got) == cap
    assert all(g[2] == step for g in got[1:-1]) and all(0 < g[2] <= step for g in got[1:])
    assert all(b[1] == a[1] + a[2] for a, b in zip(got, got[1:]))
    assert [int(rest) for key, rest in out if key == "limit"] == [len(want)]


def test_render_argument_errors(check):
    def verdict(mn=8, step=8, thr="0.2", fl="0.01", begin=0, count=96, flags=0):
        (key, *rest), = check("args", mn, step, thr, fl, begin, count, flags)
        return key if key == "ok" else rest[0]

    assert verdict() == "ok"
    assert verdict(mn=96) == "ok" and "min_spp" in verdict(mn=97)
    assert "step_spp" in verdict(step=0)
    assert verdict(mn=0, step=1, count=4095) == "ok" and "4096 rounds" in verdict(mn=0, step=1, count=4096)
    assert verdict(mn=1, step=1, count=4096) == "ok" and "4096 rounds" in verdict(mn=1, step=1, count=4097)
    for bad in ("-0.001", "nan", "inf", "-inf"):
        assert "threshold" in verdict(thr=bad), bad
        assert "floor" in verdict(fl=bad), bad
    assert verdict(thr="0", fl="0") == "ok"
    assert "FUSED" in verdict(flags=massrt.RENDER_FUSED) and "SIMPLE" in verdict(flags=massrt.RENDER_SIMPLE_TRACE)
    assert verdict(flags=massrt.RENDER_COUNTERS | massrt.RENDER_TIME_KERNELS) == "ok"
    assert verdict(begin=2 ** 32 - 1 - 96) == "ok" and "overflow" in verdict(begin=2 ** 32 - 96)
    assert verdict(mn=0, count=0) == "ok"


def test_slots_and_shard_tiles(check):
    out = check("slots")
    for key, rest in out:
        v = [int(x) for x in rest.split()]
        if key == "slot":
            x, y, i = v
            assert i == (y % 8) * 8 + x % 8
        else:
            W, H, si, sc, n = v
            assert n == adaptive_ref.tile_pixels(W, H, si, sc).shape[0] == massrt.adaptive_tile_count(W, H, si, sc)
    # the shard's tiles, slot by slot, are mrt_shard_pixels' list
    for (W, H) in SIZES:
        for si, sc in SHARDS:
            pix = adaptive_ref.tile_pixels(W, H, si, sc).reshape(-1)
            assert np.array_equal(pix[pix >= 0], massrt.shard_pixels(W, H, si, sc))


# ---- the whole rule over the oracle's frames ---------------------------------

W, H, SEED = 50, 27, 1
RULE = dict(min_spp=8, step_spp=8, cap=96, threshold=0.2, floor=0.01)
FRAME_ASPECT = W / H  # the camera of the frame's own shape


@pytest.fixture(scope="module")
def oracle_frames(golden_dir):
    o = oracle.Scene(1).builtin("sphere_grid", FRAME_ASPECT, golden_dir)
    frames = [o.render(W, H, s, 1, seed=SEED) for s in range(RULE["cap"])]
    return o, [f[0] for f in frames], [f[1] for f in frames]


def test_rule_spreads_its_samples_on_oracle_frames(oracle_frames):
    o, rgb, bo = oracle_frames
    r = adaptive_ref.run(W, H, rgb, bo, **RULE)
    counts = adaptive_ref.per_tile_counts(W, H, r["samples"])
    adaptive_ref.check_not_vacuous(counts, 8, 96)
    # what the rule does here: half the tiles stop after the first 8 samples, 4 never stop
    assert r["open"] == [14, 14, 12, 12, 12, 11, 10, 8, 6, 5, 5, 4]
    assert round(float(r["samples"].mean())) == 49
    rep = r["report"]
    assert rep["tiles"] == 28 and rep["rounds"] == len(r["open"]) == 12 and rep["spp_reached"] == 96
    assert rep["samples"] == int(r["samples"].sum()) and rep["tiles_open"] == r["open"][-1]
    assert all(a >= b for a, b in zip(r["open"], r["open"][1:]))  # a closed tile never returns
    assert int((counts == 8).sum()) == 28 - r["open"][0]
    # a pixel that stopped after c samples holds the oracle's uniform c-spp sums
    for c in np.unique(counts):
        px = np.flatnonzero(r["samples"] == c)
        want_rgb, want_b = o.render_pixels(W, H, px, 0, int(c), seed=SEED)
        assert np.array_equal(r["rgb"].reshape(-1, 3)[px].view(np.uint32), want_rgb.reshape(-1, 3).view(np.uint32)), c
        assert np.array_equal(r["bounces"][px], want_b), c
    # in two calls: capped at 40, then continued without a minimum
    a = adaptive_ref.run(W, H, rgb, bo, 8, 8, 40, 0.2, 0.01)
    b = adaptive_ref.run(W, H, rgb[40:], bo[40:], 0, 8, 56, 0.2, 0.01,
                         state=(a["rgb"], a["bounces"], a["moments"], a["samples"]))
    for k in ("rgb", "moments"):
        assert np.array_equal(b[k].view(np.uint32), r[k].view(np.uint32)), k
    assert np.array_equal(b["samples"], r["samples"]) and np.array_equal(b["bounces"], r["bounces"])
    # the display path: resolved sums are the uniform frames' means
    res = adaptive_ref.resolve(r["rgb"], r["samples"])
    px = np.flatnonzero(r["samples"] == 8)
    want = (np.float32(1.0) / np.float32(8)) * r["rgb"].reshape(-1, 3)[px]
    assert np.array_equal(res.reshape(-1, 3)[px].view(np.uint32), want.view(np.uint32))
