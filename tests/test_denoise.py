"""The Denoise display mode (main.rs:675-683, 724-747) without a GPU: the
interface (header, ctypes mirror, defaults), properties of the filter's numpy
restatement (tests/denoise_ref.py), and what the filter is for — at the
default widths it brings a low-sample-count oracle render closer to a
high-sample-count one."""
import ctypes as C
import functools
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
import massrt
import oracle
from conftest import GOLDEN, REPO

F = np.float32


# ---- interface and layout ---------------------------------------------------

def test_display_denoise_constant_and_defaults():
    assert massrt.DISPLAY_DENOISE == 4
    d = massrt.denoise_defaults()
    assert d == {"iterations": 5, "sigma_color": 2.0, "sigma_albedo": F(0.3), "sigma_normal": F(0.6)}
    assert d == {k: (v if k == "iterations" else F(v)) for k, v in denoise_ref.DEFAULTS.items()}
    p = massrt.denoise_params(iterations=2, sigma_normal=0.0)
    assert (p.iterations, p.sigma_color, p.sigma_albedo, p.sigma_normal) == (2, 2.0, F(0.3), 0.0)
    with pytest.raises(TypeError, match="sigma_colour"):
        massrt.denoise_params(sigma_colour=1.0)
    assert massrt.lib().mrt_denoise_default_params(None) != 0  # MRT_ERR_INVALID, no crash


def test_denoise_params_layout_matches_header(tmp_path):
    """ctypes mirror == the C compiler's view of mrt_denoise_params, and the
    header's MRT_DISPLAY_DENOISE is the package's."""
    if not shutil.which("gcc"):
        pytest.skip("gcc missing")
    py = massrt.MrtDenoiseParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{REPO}/include/massrt.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(mrt_denoise_params));', 'printf("mode %u\\n", MRT_DISPLAY_DENOISE);']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(mrt_denoise_params, {f}));')
    lines.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(py) == int(out.pop("size")) == 16
    assert int(out.pop("mode")) == massrt.DISPLAY_DENOISE
    assert [f for f, _ in py._fields_] == ["iterations", "sigma_color", "sigma_albedo", "sigma_normal"]
    for f, off in out.items():
        assert getattr(py, f).offset == int(off), f


# ---- the restatement --------------------------------------------------------

def test_zero_iterations_is_the_prepared_colour():
    W, H = 9, 7
    rgb, albedo, normal = denoise_ref.quirky_inputs(W, H, 1)
    c0 = denoise_ref.prepare_colour(rgb, 3)
    for aux in ({}, {"albedo": albedo, "normal": normal}):
        out = denoise_ref.denoise(W, H, rgb, 3, iterations=0, **aux)
        assert out.dtype == F and np.array_equal(out.view(np.uint32), c0.view(np.uint32))
    # the preparation's rule: NaN, negative, > 1 -> 1; -0.0 stays; everything else is (1/3) * sum
    s = np.array([np.nan, -1.0, np.inf, -0.0, 7.5, 1.5, 3.0], dtype=F)
    got = denoise_ref.prepare_colour(s, 3)
    assert np.array_equal(got[:3], [1, 1, 1]) and got[3] == 0 and np.signbit(got[3]) and got[4] == 1
    assert got[5] == (F(1.0) / F(3.0)) * F(1.5) and got[6] == 1.0  # (1/3)*3 rounds to 1.0: kept, not clamped
    assert np.array_equal(denoise_ref.prepare_albedo(np.array([np.nan, -3, np.inf, -0.0, 0.25], dtype=F)),
                          np.array([1, 0, 1, 0, 0.25], dtype=F))
    assert not denoise_ref.denoise(W, H, rgb, 0, albedo, normal).any()  # passes == 0 -> zeros


def test_constant_image_is_a_fixed_point():
    """All weights are the kernel's k (fall(0) = 1), multiples of 1/256. For a
    colour with few mantissa bits every product and partial sum is exact, so
    acc = c * sw and acc / sw = c exactly, border pixels included. For any
    other constant each of the 25 products and 25 sums of an iteration rounds
    once (2^-24 relative each, the division once more): 5 iterations stay
    within 5 * 51 * 2^-24 of it."""
    W, H = 23, 11
    a = np.full(W * H * 3, 0.5, dtype=F)
    n = np.tile(np.array([0, 0, 1], dtype=F), W * H)
    for v in (0.0, 0.25, 0.5, 0.75, 1.0):
        rgb = np.full(W * H * 3, v, dtype=F)
        assert np.array_equal(denoise_ref.denoise(W, H, rgb, 1, a, n), rgb), v
        assert np.array_equal(denoise_ref.denoise(W, H, rgb, 1), rgb), v
    rgb = np.full(W * H * 3, 0.3, dtype=F)
    out = denoise_ref.denoise(W, H, rgb, 1, a, n)
    assert np.abs(out.astype(np.float64) / np.float64(F(0.3)) - 1.0).max() <= 5 * 51 * 2.0 ** -24


def test_output_stays_in_unit_interval():
    """Prepared colour is in [0, 1]; rounding is monotone, so acc <= sw step by
    step and the quotient never exceeds 1 — for quirky inputs too, with every
    combination of terms switched off."""
    W, H = 37, 21
    rgb, albedo, normal = denoise_ref.quirky_inputs(W, H, 2)
    for kw in ({}, {"sigma_color": 0.0}, {"sigma_albedo": -1.0}, {"sigma_normal": 0.0}, {"sigma_color": 0.05}):
        for aux in ({}, {"albedo": albedo, "normal": normal}):
            out = denoise_ref.denoise(W, H, rgb, 3, **aux, **kw)
            assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0, (kw, bool(aux))


def test_guides_stop_the_blur_at_an_edge():
    """Two flat halves with different albedo: with the guides the filter does
    not mix them; colour-only at a wide sigma_color it does."""
    W, H = 32, 16
    rgb = np.zeros((H, W, 3), dtype=F)
    rgb[:, W // 2:] = 0.5
    albedo = np.where(rgb > 0, F(1.0), F(0.0)).astype(F)
    normal = np.tile(np.array([0, 0, 1], dtype=F), W * H)
    guided = denoise_ref.denoise(W, H, rgb, 1, albedo, normal, sigma_color=100.0).reshape(H, W, 3)
    assert np.array_equal(guided, rgb)  # e(a) = 3 >= sigma_albedo^2: weight 0 across the edge
    plain = denoise_ref.denoise(W, H, rgb, 1, sigma_color=100.0).reshape(H, W, 3)
    assert 0.1 < plain[H // 2, W // 2 - 1, 0] < 0.4


# ---- what the filter is for -------------------------------------------------

W_Q, H_Q = 96, 54


@functools.lru_cache(maxsize=None)
def oracle_case(scene):
    """(reference image of 1024 spp from sample 1000, albedo, normal, {spp: sums from sample 0})."""
    o = oracle.Scene(1).builtin(scene, float(massrt.ASPECT_RATIO), GOLDEN)
    ref, _ = o.render(W_Q, H_Q, 1000, 1024, seed=1)
    albedo, normal = o.prepass(W_Q, H_Q, seed=1)
    noisy = {spp: o.render(W_Q, H_Q, 0, spp, seed=1)[0] for spp in (4, 16)}
    return denoise_ref.prepare_colour(ref, 1024), albedo, normal, noisy


@pytest.mark.parametrize("spp", [4, 16])
@pytest.mark.parametrize("scene", ["cornell", "sphere_grid"])
def test_defaults_reduce_the_error_of_low_sample_counts(scene, spp):
    """err = relative L2 against the 1024-spp image over the prepared (linear,
    clamped) values; at the defaults err(denoised) <= 0.8 * err(noisy)."""
    ref, albedo, normal, noisy = oracle_case(scene)
    rgb = noisy[spp]
    e_noisy = denoise_ref.rel_l2(denoise_ref.prepare_colour(rgb, spp), ref)
    e_den = denoise_ref.rel_l2(denoise_ref.denoise(W_Q, H_Q, rgb, spp, albedo, normal), ref)
    print(f"{scene} {spp} spp: noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert e_den <= 0.8 * e_noisy, (scene, spp, e_noisy, e_den)
