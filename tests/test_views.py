"""The pixel list of a batch of views (mrt_render_views) on the host, no GPU
(csrc/host/loop.h through tools/views_check.cpp): the view list is the shard's
list once per view with v W H added, every entry splits back to its (view,
pixel), the shards of a batch cover every pixel of every view once, and the
2^32 limit on n_views W H is exact. render.hip builds its lists, and
k_generate<ViewTable> / k_refill<ViewTable> split their entries, with these functions;
on the GPU whole renders see them (tests/test_gpu_views.py)."""
import shutil
import subprocess

import pytest

from conftest import REPO

SIZES = [(2, 2), (9, 7), (21, 13), (131, 75)]
VIEWS = [1, 2, 5]
SHARDS = [1, 3]
TILE = 8  # MRT_TILE


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path_factory.mktemp("views") / "views_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(REPO / "tools" / "views_check.cpp")],
                   check=True)

    def run(mode):
        r = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
        return [ln.split() for ln in r.stdout.splitlines()]

    return run


@pytest.fixture(scope="module")
def lists(check):
    shard, views, split = {}, {}, {}
    for r in check("lists"):
        if r[0] == "shard":
            shard[tuple(int(x) for x in r[1:5])] = [int(x) for x in r[5:]]
        elif r[0] == "views":
            views[tuple(int(x) for x in r[1:6])] = [int(x) for x in r[6:]]
        else:
            assert r[0] == "split"
            split[tuple(int(x) for x in r[1:6])] = [tuple(int(y) for y in x.split(":")) for x in r[6:]]
    return shard, views, split


def shard_pixels(W, H, si, sc):
    """The shard's list as massrt.h states it: 8 x 8 tiles in raster order,
    tile t to shard t % sc, a tile's pixels in raster order."""
    tx, ty = -(-W // TILE), -(-H // TILE)
    out = []
    for t in range(si, tx * ty, sc):
        bx, by = (t % tx) * TILE, (t // tx) * TILE
        out += [y * W + x for y in range(by, by + TILE) for x in range(bx, bx + TILE) if x < W and y < H]
    return out


def test_every_case_is_there(lists):
    shard, views, split = lists
    assert set(shard) == {(W, H, sc, si) for W, H in SIZES for sc in SHARDS for si in range(sc)}
    want = {(W, H, V, sc, si) for W, H in SIZES for V in VIEWS for sc in SHARDS for si in range(sc)}
    assert set(views) == want and set(split) == want


def test_view_list_is_the_shard_list_per_view(lists):
    shard, views, _ = lists
    for (W, H, V, sc, si), got in views.items():
        base = shard[(W, H, sc, si)]
        assert base == shard_pixels(W, H, si, sc), (W, H, sc, si)
        assert got == [v * W * H + p for v in range(V) for p in base], (W, H, V, sc, si)


def test_every_entry_splits_back(lists):
    shard, views, split = lists
    for key, got in views.items():
        W, H, V, sc, si = key
        base = shard[(W, H, sc, si)]
        assert split[key] == [(v, p) for v in range(V) for p in base], key
        assert all(v < V and p < W * H and v * W * H + p == P for (v, p), P in zip(split[key], got)), key


def test_shards_cover_every_pixel_of_every_view_once(lists):
    _, views, _ = lists
    for W, H in SIZES:
        for V in VIEWS:
            for sc in SHARDS:
                union = [P for si in range(sc) for P in views[(W, H, V, sc, si)]]
                assert len(union) == V * W * H and sorted(union) == list(range(V * W * H)), (W, H, V, sc)


def test_view_struct_matches_header(tmp_path):
    """massrt.MrtView == the C compiler's view of mrt_view."""
    import ctypes as C

    import massrt
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    src = tmp_path / "view.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{REPO}/include/massrt.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(mrt_view), offsetof(mrt_view, camera), '
                   'offsetof(mrt_view, seed));return 0;}\n')
    subprocess.run(["gcc", "-o", str(tmp_path / "view"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "view")], check=True, capture_output=True, text=True).stdout.split()
    assert [C.sizeof(massrt.MrtView), massrt.MrtView.camera.offset, massrt.MrtView.seed.offset] == [int(x) for x in out]


def test_make_camera_is_the_builders_camera():
    import numpy as np

    import massrt
    b = massrt.Builder(1)
    b.add_sphere(b.material(massrt.MAT_LAMBERTIAN, b.solid(1, 1, 1)), (0, 0, 0), 1)
    b.build_bvh()
    for kw in (dict(vfov=40.0, look_from=(6, 8, 5), look_at=(0, 0, 0)),
               dict(vfov=25.0, look_from=(-3, 2, 9), look_at=(0, 1, 0), view_up=(0.1, 1, 0), aspect=1.5, aperture=0.3),
               dict(vfov=60.0, look_from=(1, 1, 1), look_at=(0, 0, 0), aperture=0.1, focus=2.5)):
        b.camera(**kw)
        _, cam = b.desc()
        got = massrt.make_camera(**kw)
        assert np.array_equal(got.fields().view(np.uint32), cam.fields().view(np.uint32)), kw


def test_limit_is_exact(check):
    rows = {tuple(int(x) for x in r[1:4]): int(r[4]) for r in check("limit") if r[0] == "fit"}
    assert len(rows) >= 12
    for (V, W, H), fits in rows.items():
        ok = V > 0 and W > 0 and H > 0 and V * W * H < 2 ** 32
        assert fits == int(ok), (V, W, H)
    assert rows[(1, 65535, 65537)] == 1 and rows[(3, 21845, 65537)] == 1  # n_views W H = 2^32 - 1: accepted
    assert rows[(1, 65536, 65536)] == 0 and rows[(2, 65536, 32768)] == 0 and rows[(4, 32768, 32768)] == 0  # 2^32: refused
    assert {V * W * H for V, W, H in rows} >= {2 ** 32 - 1, 2 ** 32}
