"""The host-only half of mrt_render_rays, no GPU: the published path stream
(mrt_path_stream) against the oracle's word for word, the renderer's own
camera rays as table entries (mrt_camera_rays) against a numpy float32
restatement (tests/rays_ref.py) bit for bit, mrt_path_ray against the header,
the argument errors of the two calls, and the work-item and limit arithmetic
of a ray list (csrc/host/loop.h through tools/rays_check.cpp). On the GPU
whole renders see them (tests/test_gpu_rays.py)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import massrt
import oracle
import rays_ref
from conftest import REPO

ASPECT = float(massrt.ASPECT_RATIO)
W, H = 48, 27
MRT_OK, MRT_ERR_INVALID = 0, 1
SKIP_MAX = 4096  # MRT_RAY_SKIP_MAX


def test_path_stream_is_the_oracles_stream():
    for seed in (0, 1, 7, 2 ** 63 + 5, 2 ** 64 - 1):
        for key in (0, 1, 2 ** 31, 2 ** 32 - 1):
            for sample in (0, 3, 2 ** 32 - 1):
                u, f = massrt.path_stream(seed, key, sample, 64)
                ou, of = oracle.path_rng(seed, key, sample, 64)
                assert np.array_equal(u, ou), (seed, key, sample)
                assert np.array_equal(f.view(np.uint32), of.view(np.uint32)), (seed, key, sample)
    assert len({tuple(massrt.path_stream(1, k, 0, 4)[0]) for k in (0, 1, 2 ** 31, 2 ** 32 - 1)}) == 4


def test_path_stream_outputs_are_optional():
    L = massrt.lib()
    u = np.zeros(8, np.uint64)
    f = np.zeros(8, np.float32)
    assert L.mrt_path_stream(5, 6, 7, 8, u.ctypes.data_as(C.POINTER(C.c_uint64)), None) == MRT_OK
    assert L.mrt_path_stream(5, 6, 7, 8, None, f.ctypes.data_as(C.POINTER(C.c_float))) == MRT_OK
    assert L.mrt_path_stream(5, 6, 7, 8, None, None) == MRT_OK
    assert L.mrt_path_stream(5, 6, 7, 0, None, None) == MRT_OK
    wu, wf = oracle.path_rng(5, 6, 7, 8)
    assert np.array_equal(u, wu) and np.array_equal(f.view(np.uint32), wf.view(np.uint32))


CAMERAS = {"pinhole": dict(vfov=40.0, look_from=(6.0, 8.0, 5.0), look_at=(0.0, 0.0, 0.0), aspect=ASPECT, aperture=0.0),
           "lens": dict(vfov=35.0, look_from=(-7.0, 5.0, 4.0), look_at=(0.0, 1.0, 0.0), aspect=ASPECT, aperture=0.1)}


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_camera_rays_equal_the_restatement(name):
    cam = massrt.make_camera(**CAMERAS[name])
    pixels = np.arange(W * H, dtype=np.uint32)
    deep = 0
    for sample in range(4):
        want = rays_ref.frame_entries(cam, W, H, seed=11, sample=sample)
        got = massrt.camera_rays(cam, W, H, pixels, seed=11, sample=sample)
        assert np.array_equal(got["key"], pixels) and np.array_equal(got["skip"], want["skip"]), (name, sample)
        assert np.array_equal(rays_ref.words(got), rays_ref.words(want)), (name, sample)
        deep += int((want["skip"] > 4).sum())  # the restatement alone: rays whose first disk try was rejected
        assert want["skip"].min() == 4 and np.all(want["skip"] % 2 == 0)
    assert deep > 4 * W * H // 10, deep  # about a fifth of the first tries are rejected (1 - pi/4)
    if name == "pinhole":  # lens_radius 0: every ray leaves the camera's origin, the disk draws are still taken
        assert np.all(got["origin"] == cam.fields()[0:3])
    else:
        assert np.unique(got["origin"], axis=0).shape[0] > W * H // 2


def test_camera_rays_take_any_pixel_list_and_seed():
    cam = massrt.make_camera(**CAMERAS["lens"])
    pixels = np.array([W * H - 1, 0, 5, 5, 700], dtype=np.uint32)
    got = massrt.camera_rays(cam, W, H, pixels, seed=2 ** 64 - 3, sample=2 ** 32 - 2)
    want = rays_ref.camera_entries(cam, W, H, pixels, seed=2 ** 64 - 3, sample=2 ** 32 - 2)
    assert np.array_equal(rays_ref.words(got), rays_ref.words(want))
    assert np.array_equal(rays_ref.words(got)[2], rays_ref.words(got)[3])


def test_path_ray_struct_matches_header(tmp_path):
    """massrt.MrtPathRay and PATH_RAY_DTYPE == the C compiler's view of mrt_path_ray: 32 B."""
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    fields = ["origin", "direction", "key", "skip"]
    src = tmp_path / "ray.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{REPO}/include/massrt.h"\n'
                   'int main(void){printf("%zu %u", sizeof(mrt_path_ray), MRT_RAY_SKIP_MAX);'
                   + "".join(f'printf(" %zu", offsetof(mrt_path_ray, {f}));' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "ray"), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "ray")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out == [32, SKIP_MAX, 0, 12, 24, 28]
    assert C.sizeof(massrt.MrtPathRay) == 32 == massrt.PATH_RAY_DTYPE.itemsize
    assert [getattr(massrt.MrtPathRay, f).offset for f in fields] == out[2:]
    assert [massrt.PATH_RAY_DTYPE.fields[f][1] for f in fields] == out[2:]
    assert massrt.RAY_SKIP_MAX == SKIP_MAX


def test_host_call_argument_errors():
    L = massrt.lib()
    cam = massrt.make_camera(**CAMERAS["pinhole"])
    px = np.array([0, 1, W * H - 1], dtype=np.uint32)
    ppx = px.ctypes.data_as(C.POINTER(C.c_uint32))
    out = (massrt.MrtPathRay * 3)()
    before = bytes(out)

    def err(rc, text):
        assert rc == MRT_ERR_INVALID and text in L.mrt_global_last_error().decode(), (rc, L.mrt_global_last_error())
        assert bytes(out) == before  # a refused call writes nothing

    err(L.mrt_camera_rays(None, W, H, ppx, 3, 1, 0, out), "null camera")
    err(L.mrt_camera_rays(C.byref(cam), 0, H, ppx, 3, 1, 0, out), "image size")
    err(L.mrt_camera_rays(C.byref(cam), W, 0, ppx, 3, 1, 0, out), "image size")
    err(L.mrt_camera_rays(C.byref(cam), 65536, 65536, ppx, 3, 1, 0, out), "image size")
    err(L.mrt_camera_rays(C.byref(cam), W, H, None, 3, 1, 0, out), "null pixels or output")
    err(L.mrt_camera_rays(C.byref(cam), W, H, ppx, 3, 1, 0, None), "null pixels or output")
    bad = np.array([0, W * H, 1], dtype=np.uint32)  # one past the last pixel
    err(L.mrt_camera_rays(C.byref(cam), W, H, bad.ctypes.data_as(C.POINTER(C.c_uint32)), 3, 1, 0, out), "outside")
    assert L.mrt_camera_rays(C.byref(cam), W, H, None, 0, 1, 0, None) == MRT_OK  # no pixels: nothing to write
    assert bytes(out) == before
    assert L.mrt_camera_rays(C.byref(cam), W, H, ppx, 3, 1, 0, out) == MRT_OK
    assert [r.key for r in out] == [0, 1, W * H - 1]
    with pytest.raises(massrt.MassrtError, match="outside"):
        massrt.camera_rays(cam, W, H, [W * H])
    with pytest.raises(ValueError, match="PATH_RAY_DTYPE"):
        massrt.path_rays(np.zeros((3, 8), np.float32))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = tmp_path_factory.mktemp("rays") / "rays_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(REPO / "tools" / "rays_check.cpp")],
                   check=True)

    def run(mode):
        r = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
        return [ln.split() for ln in r.stdout.splitlines()]

    return run


def test_work_items_split_sample_minor(check):
    rows = [[int(x) for x in r[1:]] for r in check("work") if r[0] == "work"]
    assert len(rows) >= 50 and {r[0] for r in rows} == {1, 3, 5, 16, 1024}
    for spp, g, i, s in rows:
        assert (i, s) == divmod(g, spp), (spp, g)
    assert any(g == 2 ** 32 - 1 for _, g, _, _ in rows)


def test_skip_clamp_and_host_check(check):
    rows = check("skip")
    clamp = {int(r[1]): int(r[2]) for r in rows if r[0] == "clamp"}
    assert clamp == {s: min(s, SKIP_MAX) for s in clamp} and {SKIP_MAX - 1, SKIP_MAX, SKIP_MAX + 1, 2 ** 32 - 1} <= set(clamp)
    bad = [(int(r[1]), int(r[2])) for r in rows if r[0] == "bad"]
    # tables of 5 (one entry at the limit itself, which is allowed): none bad -> 5, else the first bad position
    assert bad == [(0, 5), (1, 0), (1, 4), (2, 2), (2, 0), (0, 0)]


def test_sample_range_limit(check):
    rows = {(int(r[1]), int(r[2])): int(r[3]) for r in check("fit") if r[0] == "fit"}
    assert len(rows) >= 10
    for (b, n), fits in rows.items():
        assert fits == int(b + n <= 2 ** 32 - 1), (b, n)
    assert rows[(1, 2 ** 32 - 2)] == 1 and rows[(1, 2 ** 32 - 1)] == 0
