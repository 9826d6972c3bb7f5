"""The renderer's own camera rays as mrt_path_ray entries, restated in numpy
float32 from include/massrt.h's text (mrt_camera_rays) and the formulas of
camera_ray, camera_ray_uv and random_in_unit_disk (csrc/device/material.h;
main.rs:258-260, world.rs:53-63, math.rs:277-291). The draws come from the
oracle's path stream; no function of the library under test is called.
Every operation is one IEEE f32 operation on float32 arrays, in the order the
formulas are written (numpy never contracts a multiply and an add)."""
import numpy as np

import massrt
import oracle

F = np.float32
TRIES = 24  # disk tries drawn per ray; (1 - pi/4)^24 ~ 1e-16 that a ray needs more (asserted)


def camera_entries(cam, W, H, pixels, seed, sample):
    """PATH_RAY_DTYPE entries of `pixels` (p = y*W + x) for `sample`: the ray,
    key = p, skip = 2 (jitter) + 2 per try of random_in_unit_disk."""
    f = cam.fields()
    origin, llc, hor, ver, cu, cv, lens = f[0:3], f[3:6], f[6:9], f[9:12], f[12:15], f[15:18], f[18]
    px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    n = px.size
    d = np.stack([oracle.path_rng(seed, int(p), sample, 2 + 2 * TRIES)[1] for p in px]).astype(F)
    x, y = (px % np.uint32(W)).astype(F), (px // np.uint32(W)).astype(F)
    u = (x + d[:, 0]) / F(W - 1)
    v = (y + d[:, 1]) / F(H - 1)
    bx, by = np.zeros(n, F), np.zeros(n, F)
    skip = np.full(n, 2, np.uint32)
    open_ = np.ones(n, bool)
    for t in range(TRIES):
        xs = d[:, 2 + 2 * t] * F(2.0) - F(1.0)
        ys = d[:, 3 + 2 * t] * F(2.0) - F(1.0)
        skip[open_] += 2
        ok = open_ & ~(((xs * xs + ys * ys) + F(0.0) * F(0.0)) >= F(1.0))
        bx[ok], by[ok] = xs[ok], ys[ok]
        open_ &= ~ok
    assert not open_.any(), "a ray needed more than TRIES disk tries"
    blur_x, blur_y = bx * lens, by * lens
    out = np.zeros(n, dtype=massrt.PATH_RAY_DTYPE)
    for c in range(3):
        offset = cu[c] * blur_x + cv[c] * blur_y
        out["origin"][:, c] = origin[c] + offset
        out["direction"][:, c] = (((llc[c] + hor[c] * u) + ver[c] * v) - origin[c]) - offset
    out["key"] = px
    out["skip"] = skip
    assert out["origin"].dtype == F and u.dtype == F and blur_x.dtype == F
    return out


def frame_entries(cam, W, H, seed, sample):
    """camera_entries of every pixel of a W x H frame, in pixel order."""
    return camera_entries(cam, W, H, np.arange(W * H, dtype=np.uint32), seed, sample)


def words(entries):
    """The entries as uint32 words [n, 8], for bit-for-bit comparison."""
    return np.ascontiguousarray(entries).view(np.uint32).reshape(-1, 8)
