"""numpy float32 restatement of the Denoise view's guided à-trous filter, as
include/massrt.h states it (mrt_denoise_device). Written from that text, not
from the kernel: whole-image arrays shifted per tap, taps outside the image
skipped, dy outer and dx inner, every operation a float32 one in the stated
order. A helper: pytest does not collect it."""
import numpy as np

F = np.float32
DEFAULTS = {"iterations": 5, "sigma_color": 2.0, "sigma_albedo": 0.3, "sigma_normal": 0.6}
H_TAPS = (F(3.0) / F(8.0), F(1.0) / F(4.0), F(1.0) / F(16.0))


def prepare_colour(rgb, passes):
    """c0, (H, W, 3): v = (1/passes) * sum; NaN, negative and > 1 -> 1."""
    with np.errstate(all="ignore"):
        v = (F(1.0) / F(passes)) * np.asarray(rgb, dtype=F)
        return np.where(~(v >= F(0.0)) | (v > F(1.0)), F(1.0), v).astype(F)


def prepare_albedo(albedo):
    """Rust p.min(1).max(0): the non-NaN operand wins, so NaN -> 1 (np.clip would keep it)."""
    a = np.asarray(albedo, dtype=F)
    with np.errstate(invalid="ignore"):
        m = np.where(np.isnan(a), F(1.0), np.where(a < F(1.0), a, F(1.0)))  # a.min(1)
        return np.where(m > F(0.0), m, F(0.0)).astype(F)  # .max(0): m is never NaN; -0.0 > 0 is false -> +0.0


def _fall(t):
    with np.errstate(all="ignore"):
        u = F(1.0) - t
        return np.where(t < F(1.0), u * u, F(0.0)).astype(F)  # NaN -> 0


def _dist(uq, up):
    with np.errstate(all="ignore"):
        d = uq - up
        return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F)


def _inv(sigma):
    """1 / sigma^2 in f32, or None where sigma <= 0 switches the term off."""
    sigma = F(sigma)
    if not sigma > F(0.0):
        return None
    with np.errstate(all="ignore"):
        return F(1.0) / (sigma * sigma)


def denoise(width, height, rgb, passes, albedo=None, normal=None, iterations=5, sigma_color=2.0, sigma_albedo=0.3,
            sigma_normal=0.6):
    """W*H*3 float32 in the accumulation buffers' pixel order (p = y*W + x)."""
    W, H = int(width), int(height)
    if passes == 0:
        return np.zeros(W * H * 3, dtype=F)
    c = prepare_colour(np.asarray(rgb, dtype=F).reshape(H, W, 3), passes)
    aux = albedo is not None
    if aux:
        a = prepare_albedo(np.asarray(albedo, dtype=F).reshape(H, W, 3))
        n = np.asarray(normal, dtype=F).reshape(H, W, 3)
    inv_a = _inv(sigma_albedo) if aux else None
    inv_n = _inv(sigma_normal) if aux else None
    for i in range(int(iterations)):
        s = 1 << i
        with np.errstate(all="ignore"):
            inv_c = _inv(F(sigma_color) * F(2.0 ** -i))
        acc = np.zeros((H, W, 3), dtype=F)
        sw = np.zeros((H, W), dtype=F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = F(H_TAPS[abs(dx)] * H_TAPS[abs(dy)])
                # pixels p = (x, y) whose tap q = (x + dx*s, y + dy*s) lies inside the image
                x0, x1 = max(0, -dx * s), min(W, W - dx * s)
                y0, y1 = max(0, -dy * s), min(H, H - dy * s)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                if dx == 0 and dy == 0:
                    w = np.full((H, W), k, dtype=F)
                else:
                    w = np.full((y1 - y0, x1 - x0), k, dtype=F)
                    with np.errstate(all="ignore"):
                        if inv_c is not None:
                            w = (w * _fall(_dist(c[Q], c[P]) * inv_c)).astype(F)
                        if inv_a is not None:
                            w = (w * _fall(_dist(a[Q], a[P]) * inv_a)).astype(F)
                        if inv_n is not None:
                            w = (w * _fall(_dist(n[Q], n[P]) * inv_n)).astype(F)
                acc[P] = acc[P] + w[..., None] * c[Q]
                sw[P] = sw[P] + w
        c = (acc / sw[..., None]).astype(F)
    return c.reshape(-1)


def rel_l2(x, ref):
    """Relative L2 distance of two prepared images (float64 accumulation)."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def quirky_inputs(W, H, seed):
    """Colour sums (for passes = 3), albedo and normal with every special case
    the preparation names sprinkled in."""
    rng = np.random.default_rng(seed)
    n = W * H * 3
    rgb = (rng.random(n, dtype=F) * F(3.6)).astype(F)  # mostly in [0, 1] after / 3, some above
    albedo = (rng.random(n, dtype=F) * F(1.4) - F(0.2)).astype(F)  # some outside [0, 1]
    normal = rng.standard_normal((W * H, 3)).astype(F)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(F)
    normal = normal.reshape(-1)
    for arr, specials in ((rgb, [np.nan, -1.0, np.inf, -0.0, 7.5, -np.inf]), (albedo, [np.nan, -3.0, np.inf, -0.0, 2.0]),
                          (normal, [np.nan])):
        for v in specials:
            arr[rng.integers(0, n, size=max(1, n // 40))] = F(v)
    miss = rng.integers(0, W * H, size=max(1, W * H // 10))  # zero normals: rays that missed
    normal.reshape(-1, 3)[miss] = F(0.0)
    return rgb, albedo, normal
