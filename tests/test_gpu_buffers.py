"""The context's device buffers (csrc/device/devmem.h DevBuf) through the C
ABI: buffers that grow with a call's size, the scene allocation replaced by a
second upload, the path pool split again for another queue count, and an
Image's buffers made and released twice on one context. A buffer that kept a
stale size or pointer would show as a result that differs from what a fresh
context, which made only that one call, returns. Equal means equal as uint32
bit patterns. No test provokes an error path on the device."""
import numpy as np
import pytest

import massrt
from conftest import GOLDEN
from ray_gen import camera_rays

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "cornell_smoke")  # without volumes (ln_table null) and with (the 32 MiB table, traversal draws)


@pytest.fixture(scope="module")
def builders():
    return {name: massrt.Builder(1).builtin(name, float(massrt.ASPECT_RATIO), GOLDEN) for name in SCENES}


def bits(a):
    """The array's bytes as uint32 words (display bytes stay bytes)."""
    a = np.ascontiguousarray(a)
    raw = a.reshape(-1).view(np.uint8)
    return raw.view(np.uint32) if a.dtype.itemsize % 4 == 0 else raw


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def fresh(builder, call):
    """`call(ctx)` on a new context that holds `builder`'s scene (None: no scene) and makes no other call."""
    c = massrt.Context(0)
    try:
        if builder is not None:
            c.upload(builder)
        return call(c)
    finally:
        c.close()


@pytest.mark.parametrize("name", SCENES)
def test_ray_buffers_regrow(builders, name):
    b = builders[name]
    _, cam = b.desc()
    rays = camera_rays(cam, 4096, 5)
    sets = (rays[:64], rays, rays[:64])  # the ray buffers grow for the second call and are kept for the third
    for method in ("trace_rays", "shade_rays"):
        want = [fresh(b, lambda c: getattr(c, method)(r)) for r in sets[:2]]
        c = massrt.Context(0)
        c.upload(b)
        got = [getattr(c, method)(r) for r in sets]
        c.close()
        assert [len(g) for g in got] == [64, 4096, 64], method
        assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[0]), method
        assert same(got[2], got[0]), method


@pytest.mark.parametrize("name", SCENES)
def test_frame_buffers_regrow(builders, name):
    b = builders[name]
    sizes = ((16, 16), (64, 40), (16, 16))  # staging, lane-ray slots and the denoise scratch grow, then are kept
    want = {}
    for W, H in sizes[:2]:
        rgb, bo = fresh(b, lambda c: c.render(W, H, 0, 2, seed=3))
        alb, nrm = fresh(b, lambda c: c.prepass(W, H, seed=1))
        want[W, H] = {
            "render": (rgb, bo),
            "prepass": (alb, nrm),
            "default": fresh(None, lambda c: c.tonemap(W, H, rgb, bo, 2, massrt.DISPLAY_DEFAULT)),
            "depth": fresh(None, lambda c: c.tonemap(W, H, rgb, bo, 2, massrt.DISPLAY_DEPTH)),
            "denoise": fresh(None, lambda c: c.denoise(W, H, rgb, 2, alb, nrm, iterations=2)),
        }
    c = massrt.Context(0)
    c.upload(b)
    for W, H in sizes:
        w = want[W, H]
        rgb, bo = c.render(W, H, 0, 2, seed=3)
        assert same(rgb, w["render"][0]) and same(bo, w["render"][1]), (W, H)
        alb, nrm = c.prepass(W, H, seed=1)
        assert same(alb, w["prepass"][0]) and same(nrm, w["prepass"][1]), (W, H)
        assert same(c.tonemap(W, H, rgb, bo, 2, massrt.DISPLAY_DEFAULT), w["default"]), (W, H)
        assert same(c.tonemap(W, H, rgb, bo, 2, massrt.DISPLAY_DEPTH), w["depth"]), (W, H)
        assert same(c.denoise(W, H, rgb, 2, alb, nrm, iterations=2), w["denoise"]), (W, H)
    c.close()
    assert bits(want[64, 40]["render"][0]).any() and want[64, 40]["default"].any()  # not a comparison of zeros


def test_scene_replaced(builders):
    W, H = 32, 24

    def look(c):
        return c.render(W, H, 0, 1, seed=2), c.scene_bytes()

    want = {name: fresh(builders[name], look) for name in SCENES}
    assert want["cornell"][1] < (1 << 20) and want["cornell_smoke"][1] > (32 << 20)  # only the volume scene carries the ln table
    c = massrt.Context(0)
    for name in ("cornell_smoke", "cornell", "cornell_smoke"):
        c.upload(builders[name])
        (rgb, bo), nbytes = look(c)
        assert same(rgb, want[name][0][0]) and same(bo, want[name][0][1]), name
        assert nbytes == want[name][1], name
    c.close()


def test_queue_count_reallocates_the_pool(builders):
    """The sums are per pixel in sample order, so the image cannot depend on how the pool is split."""
    W, H = 48, 32
    c = massrt.Context(0)
    c.upload(builders["cornell_smoke"])
    first = c.render(W, H, 0, 4, seed=5)
    assert bits(first[0]).any()
    for queues in (1, 3):
        c.set_option("queues", queues)
        assert c.tuning()["queues"] == queues
        rgb, bo = c.render(W, H, 0, 4, seed=5)
        assert same(rgb, first[0]) and same(bo, first[1]), queues
    c.close()


def test_image_lifecycle(builders):
    W, H = 40, 24
    c = massrt.Context(devices=[0, 0])
    c.upload(builders["cornell_smoke"])
    rounds = []
    for _ in range(2):
        img = massrt.Image(c, W, H)
        img.render(3, 0, 2)
        img.prepass(1)
        shown = img.tonemap(massrt.DISPLAY_DENOISE)
        rgb, bo, passes = img.read()
        img.close()
        assert passes == 2 and bits(rgb).any() and shown.any()
        rounds.append((shown, rgb, bo))
    for a, b in zip(*rounds):
        assert same(a, b)
    c.close()  # succeeds only once both images are closed (mrt_destroy counts them)
    assert c.h is None
