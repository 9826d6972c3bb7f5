"""The Denoise display mode on the device (csrc/device/denoise.hip): the
filtered floats equal the numpy restatement (tests/denoise_ref.py) bit for
bit, 0 iterations give Default's bytes (the reference's own Denoise mode
without its `denoise` feature), the image path follows its pre-pass and its
parameters, and every invalid call is refused."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref
import massrt

pytestmark = pytest.mark.gpu
F = np.float32
ASPECT = float(massrt.ASPECT_RATIO)
MRT_ERR_INVALID = 1


@pytest.fixture(scope="module")
def dctx():
    c = massrt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell(golden_dir):
    c = massrt.Context(0)
    c.upload(massrt.Builder(1).builtin("cornell", ASPECT, golden_dir))
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def inputs(W, H):
    return denoise_ref.quirky_inputs(W, H, 7 * W + H)


# ---- bit-exact floats against the restatement --------------------------------
# 1x1: only the centre tap; 5x3: smaller than one window; 37x21: odd and
# smaller than 2*16, so at steps 8 and 16 most taps fall outside; 130x70:
# several 64x4 workgroups both ways plus ragged edges.

@pytest.mark.parametrize("aux", [False, True], ids=["colour", "guided"])
@pytest.mark.parametrize("iterations", [0, 1, 2, 5])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 21), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_floats_equal_the_restatement(dctx, size, iterations, aux):
    W, H = size
    rgb, albedo, normal = inputs(W, H)
    kw = {"albedo": albedo, "normal": normal} if aux else {}
    got = dctx.denoise(W, H, rgb, 3, iterations=iterations, **kw)
    exp = denoise_ref.denoise(W, H, rgb, 3, iterations=iterations, **kw)
    assert got.dtype == F and got.shape == (W * H * 3,)
    bad = np.flatnonzero(_bits(got) != _bits(exp))
    assert bad.size == 0, (bad[:8], got[bad[:8]], exp[bad[:8]])


@pytest.mark.parametrize("off", ["sigma_color", "sigma_albedo", "sigma_normal"])
@pytest.mark.parametrize("value", [0.0, -1.0])
def test_a_sigma_at_or_below_zero_switches_its_term_off(dctx, off, value):
    W, H = 37, 21
    rgb, albedo, normal = inputs(W, H)
    got = dctx.denoise(W, H, rgb, 3, albedo, normal, iterations=3, **{off: value})
    exp = denoise_ref.denoise(W, H, rgb, 3, albedo, normal, iterations=3, **{off: value})
    assert np.array_equal(_bits(got), _bits(exp))
    if off != "sigma_color":  # both guide terms off == no guides at all
        other = "sigma_normal" if off == "sigma_albedo" else "sigma_albedo"
        both = dctx.denoise(W, H, rgb, 3, albedo, normal, iterations=3, **{off: value, other: value})
        assert np.array_equal(_bits(both), _bits(dctx.denoise(W, H, rgb, 3, iterations=3)))


def test_other_widths_and_zero_passes(dctx):
    W, H = 37, 21
    rgb, albedo, normal = inputs(W, H)
    for kw in ({"sigma_color": 0.1, "sigma_albedo": 5.0, "sigma_normal": 0.05}, {"sigma_color": float("inf")},
               {"iterations": 8, "sigma_color": 1e-30}):  # 1e-30^2 underflows: inv = inf, 0 * inf = NaN -> weight 0
        got = dctx.denoise(W, H, rgb, 3, albedo, normal, **kw)
        assert np.array_equal(_bits(got), _bits(denoise_ref.denoise(W, H, rgb, 3, albedo, normal, **kw))), kw
    assert not dctx.denoise(W, H, rgb, 0, albedo, normal).any()  # main.rs:647
    assert not dctx.denoise(W, H, rgb, 0, iterations=0).any()


def test_device_entry_on_a_stream_equals_the_host_entry(dctx):
    """mrt_denoise_device on the caller's stream, scratch buffers reused at a
    smaller size after a larger one."""
    import torch

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    for W, H in ((130, 70), (37, 21)):
        rgb, albedo, normal = inputs(W, H)
        t_rgb, t_a, t_n = (torch.from_numpy(x).to(dev) for x in (rgb, albedo, normal))
        out = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for aux in (True, False):
            dctx.denoise_device(W, H, t_rgb.data_ptr(), 3, t_a.data_ptr() if aux else None,
                                t_n.data_ptr() if aux else None, out.data_ptr(), s.cuda_stream, iterations=4)
            s.synchronize()
            exp = dctx.denoise(W, H, rgb, 3, *((albedo, normal) if aux else ()), iterations=4)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(exp)), (W, H, aux)


# ---- the anchor to the reference --------------------------------------------

def test_zero_iterations_give_default_bytes(dctx, cornell):
    """Feature `denoise` off: denoise() is a no-op and Denoise == Default
    (main.rs:675-683, 724-747). The byte of the prepared colour is Default's
    byte for every input, the quirks of tests/test_tonemap.py included."""
    W, H = 4, 2
    rgb = np.array([0.0, 1.0, 2.0, 0.5, 0.25, 4.0, np.nan, -1.0, np.inf, 1e-30, 3.0, 0.9999,
                    0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2], dtype=F)
    b = np.arange(8, dtype=np.uint32)
    for passes in (1, 2, 3):
        den = dctx.denoise(W, H, rgb, passes, iterations=0)
        assert np.array_equal(dctx.tonemap(W, H, den, b, 1, massrt.DISPLAY_DEFAULT),
                              dctx.tonemap(W, H, rgb, b, passes, massrt.DISPLAY_DEFAULT))
    W, H = 37, 21
    rgb, albedo, normal = inputs(W, H)
    b = np.zeros(W * H, np.uint32)
    den = dctx.denoise(W, H, rgb, 3, albedo, normal, iterations=0)
    assert np.array_equal(dctx.tonemap(W, H, den, b, 1), dctx.tonemap(W, H, rgb, b, 3))
    W, H = 64, 36
    rgb, b = cornell.render(W, H, 0, 4, seed=1)
    a, n = cornell.prepass(W, H, seed=1)
    den = cornell.denoise(W, H, rgb, 4, a, n, iterations=0)
    assert np.array_equal(cornell.tonemap(W, H, den, b, 1), cornell.tonemap(W, H, rgb, b, 4))


# ---- the image path -----------------------------------------------------------

def _image_views(c):
    """Denoise views of a Cornell 64x36 x 4 spp image on context c: before a
    pre-pass, after it, after set_denoise, and cleared."""
    W, H = 64, 36
    img = massrt.Image(c, W, H)
    img.render(1, 0, 4)
    views = [img.tonemap(massrt.DISPLAY_DENOISE)]
    img.prepass(1)
    views.append(img.tonemap(massrt.DISPLAY_DENOISE))
    img.set_denoise(iterations=2, sigma_color=1.0, sigma_normal=0.0)
    views.append(img.tonemap(massrt.DISPLAY_DENOISE))
    img.set_denoise()  # back to the defaults
    views.append(img.tonemap(massrt.DISPLAY_DENOISE))
    rgb, b, passes = img.read()
    default = img.tonemap(massrt.DISPLAY_DEFAULT)
    img.clear()
    views.append(img.tonemap(massrt.DISPLAY_DENOISE))
    img.close()
    return views, (rgb, b, passes), default


def test_image_denoise_view(cornell, golden_dir):
    W, H = 64, 36
    c = cornell
    views, (rgb, b, passes), default = _image_views(c)
    assert passes == 4
    a, n = c.prepass(W, H, seed=1)
    byte = lambda den: c.tonemap(W, H, den, b, 1, massrt.DISPLAY_DEFAULT)
    assert np.array_equal(views[0], byte(c.denoise(W, H, rgb, 4)))  # colour-only before a pre-pass
    assert np.array_equal(views[1], byte(c.denoise(W, H, rgb, 4, a, n)))
    assert np.array_equal(views[2], byte(c.denoise(W, H, rgb, 4, a, n, iterations=2, sigma_color=1.0,
                                                   sigma_normal=0.0)))
    assert np.array_equal(views[3], views[1])
    assert views[4].shape == (H, W, 3) and not views[4].any()  # pass count 0 (main.rs:647)
    # the views differ from each other and from Default: the filter did run
    assert not np.array_equal(views[0], views[1]) and not np.array_equal(views[1], views[2])
    assert not np.array_equal(views[1], default)
    # the restatement gives the same floats, hence the same bytes
    assert np.array_equal(views[1], byte(denoise_ref.denoise(W, H, rgb, 4, a, n)))
    # one context over two device slots: the tiles are gathered first, same bytes
    multi = massrt.Context(devices=[0, 0])
    multi.upload(massrt.Builder(1).builtin("cornell", ASPECT, golden_dir))
    mviews, _, mdefault = _image_views(multi)
    multi.close()
    assert np.array_equal(mdefault, default)
    for k, (v, m) in enumerate(zip(views, mviews)):
        assert np.array_equal(v, m), k


def test_image_set_denoise_rejects_bad_params(cornell):
    img = massrt.Image(cornell, 8, 8)
    for kw in ({"iterations": 9}, {"sigma_color": float("nan")}, {"sigma_albedo": float("nan")},
               {"sigma_normal": float("nan")}):
        with pytest.raises(massrt.MassrtError, match="denoise"):
            img.set_denoise(**kw)
    with pytest.raises(massrt.MassrtError, match="bad display mode"):
        img.tonemap(5)
    img.close()


# ---- quality on the device ----------------------------------------------------

def test_defaults_reduce_the_error_on_device_renders(cornell):
    """The CPU condition of tests/test_denoise.py at cornell 16 spp, every
    image rendered and filtered on the device (the same sample streams)."""
    W, H = 96, 54
    ref, _ = cornell.render(W, H, 1000, 1024, seed=1)
    ref = denoise_ref.prepare_colour(ref, 1024)
    rgb, _ = cornell.render(W, H, 0, 16, seed=1)
    a, n = cornell.prepass(W, H, seed=1)
    e_noisy = denoise_ref.rel_l2(denoise_ref.prepare_colour(rgb, 16), ref)
    e_den = denoise_ref.rel_l2(cornell.denoise(W, H, rgb, 16, a, n), ref)
    print(f"cornell 16 spp on the device: noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert e_den <= 0.8 * e_noisy, (e_noisy, e_den)


# ---- errors -------------------------------------------------------------------

def test_invalid_calls_are_refused(dctx):
    L = massrt.lib()
    W, H = 5, 3
    rgb, albedo, normal = (np.ascontiguousarray(x) for x in inputs(W, H))
    out = np.empty(W * H * 3, dtype=F)
    fp = massrt._fptr

    def host(w=W, h=H, c=rgb, a=albedo, n=normal, o=out, **kw):
        p = massrt.MrtDenoiseParams(kw.get("iterations", 5), kw.get("sigma_color", 2.0), kw.get("sigma_albedo", 0.3),
                                    kw.get("sigma_normal", 0.6))
        ptr = lambda x: None if x is None else fp(x)
        return L.mrt_denoise(dctx.h, w, h, ptr(c), 3, ptr(a), ptr(n), C.byref(p), ptr(o))

    assert host() == 0
    assert L.mrt_denoise(dctx.h, W, H, fp(rgb), 3, fp(albedo), fp(normal), None, fp(out)) == 0  # NULL = defaults
    assert np.array_equal(_bits(out), _bits(denoise_ref.denoise(W, H, rgb, 3, albedo, normal)))
    bad = {"zero width": dict(w=0), "zero height": dict(h=0), "iterations > 8": dict(iterations=9),
           "NaN sigma_color": dict(sigma_color=float("nan")), "NaN sigma_albedo": dict(sigma_albedo=float("nan")),
           "NaN sigma_normal": dict(sigma_normal=float("nan")), "null colour": dict(c=None), "null output": dict(o=None),
           "albedo only": dict(n=None), "normal only": dict(a=None), "out == colour": dict(o=rgb),
           "out == albedo": dict(o=albedo), "out == normal": dict(o=normal)}
    for what, kw in bad.items():
        assert host(**kw) == MRT_ERR_INVALID, what
        assert L.mrt_last_error(dctx.h), what
    assert host(iterations=8) == 0  # the bound itself is allowed

    # the same checks in the _device entry point, on device memory
    import torch

    dev = torch.device("cuda", 0)
    t_rgb, t_a, t_n = (torch.from_numpy(x).to(dev) for x in (rgb, albedo, normal))
    t_out = torch.empty(W * H * 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def device(w=W, h=H, c=t_rgb, a=t_a, n=t_n, o=t_out, **kw):
        ptr = lambda x: None if x is None else x.data_ptr()
        try:
            dctx.denoise_device(w, h, ptr(c) or 0, 3, ptr(a), ptr(n), ptr(o) or 0, None, **kw)
        except massrt.MassrtError as e:
            return str(e)
        return ""

    assert device() == ""
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t_out.cpu().numpy()), _bits(out))
    for what, kw in bad.items():
        kw = {k: {id(rgb): t_rgb, id(albedo): t_a, id(normal): t_n}.get(id(v), v) for k, v in kw.items()}
        assert device(**kw) != "", what

    # mrt_tonemap(_device) has no albedo/normal inputs: mode 4 stays rejected
    with pytest.raises(massrt.MassrtError, match="bad display mode"):
        dctx.tonemap(W, H, rgb, np.zeros(W * H, np.uint32), 3, massrt.DISPLAY_DENOISE)
