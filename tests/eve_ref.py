"""EveMaterial and the mapped normal, restated in numpy float32.

Written from the reference's text, not from the library's C++:
  Texture::get_f + WrapMode::Repeat   texture.rs:126-148, 283-291
  EveMaterial::{normal_occlusion, albedo_roughness, pmdg, scatter, emit}   eve.rs:66-128
  EveMaterialColor::get               eve.rs:190-198
  Triangle::with_norms_and_uvs        geom.rs:468-496 (tangent, bitangent)
  Triangle::intersect's hit record    geom.rs:535-584 (barycentrics, normal, uv, mapped normal)
  Hit::set_face_normal                geom.rs:17-24
  Instance::intersect                 geom.rs:405-419 (ray in, point and normal out)
Every function works on arrays of N hits; every operation is one IEEE f32
operation in the reference's order (numpy does not contract a*b+c), so the
device result must equal these bits. Vector operators follow generic.rs:
dot = (x*x' + y*y') + z*z', M4 * v = ((c0*x + c1*y) + c2*z) + c3*w.
"""
import numpy as np

f32 = np.float32
ONE, TWO = f32(1.0), f32(2.0)


def _a(x):
    return np.asarray(x, dtype=f32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def length(a):
    return np.sqrt(dot(a, a))


def unit(a):
    return a / length(a)[..., None]


def reflect(v, n):
    """V3::reflect (math.rs): v - n * v.dot(n) * 2.0"""
    return v - (n * dot(v, n)[..., None]) * TWO


def transform(m16, p, w):
    """M4::transform (generic.rs:105-115) of column-major matrices [N, 16] (or [16])."""
    m = _a(m16).reshape(-1, 4, 4)  # [N, column, row]
    c = [m[:, k, :3] for k in range(4)]
    return ((c[0] * p[..., 0:1] + c[1] * p[..., 1:2]) + c[2] * p[..., 2:3]) + c[3] * f32(w)


def _fract(x):
    return x - np.trunc(x)


def _usize(x, top):
    """`f32 as usize` (saturating, NaN -> 0), then the index the reference
    would panic beyond held at the last texel."""
    with np.errstate(invalid="ignore"):
        i = np.where(x > 0, x, 0).astype(np.int64)
    return np.minimum(i, top)


def get_f(tex, uv):
    """Texture::get_f with WrapMode::Repeat. tex: uint8 [H, W, 4], row 0 first; uv: [N, 2] -> [N, 4]."""
    tex = np.asarray(tex, dtype=np.uint8)
    H, W = tex.shape[:2]
    px = tex.astype(f32) / f32(255.0)  # texture.rs:44
    uv = _a(uv)
    x, y = uv[:, 0], uv[:, 1]
    x = np.where(x < 0, ONE - _fract(np.abs(x)), x)
    y = np.where(y < 0, ONE - _fract(np.abs(y)), y)
    x = np.where(x > 1, _fract(x), x)
    y = np.where(y > 1, _fract(y), y)
    x = x * f32(W - 1)
    y = y * f32(H - 1)
    x0, x1 = _usize(np.floor(x), W - 1), _usize(np.ceil(x), W - 1)
    y0, y1 = _usize(np.floor(y), H - 1), _usize(np.ceil(y), H - 1)
    t = (x - x0.astype(f32))[:, None]
    p0 = px[y0, x0] * (ONE - t) + px[y0, x1] * t
    p1 = px[y1, x0] * (ONE - t) + px[y1, x1] * t
    t = (y - y0.astype(f32))[:, None]
    return p1 * t + p0 * (ONE - t)


def normal_occlusion(no_tex, uv):
    """EveMaterial::normal_occlusion (eve.rs:66-73): the tangent-space normal [N, 3]."""
    p = get_f(no_tex, uv) * TWO - ONE
    x = (ONE - p[:, 1] * p[:, 1]) - p[:, 3] * p[:, 3]
    z = np.sqrt(np.abs(x))
    return unit(np.stack([p[:, 1], p[:, 3], z], axis=-1))


def palette(colors, i):
    """EveMaterialColor::get (eve.rs:190-198). colors: [4, 3]; i: [N] -> [N, 3]."""
    colors = _a(colors).reshape(4, 3)
    i = _a(i) * f32(3.0)
    i0 = _usize(np.floor(i), 3)
    i1 = _usize(np.ceil(i), 3)
    t = (i - i0.astype(f32))[:, None]
    return colors[i0] * (ONE - t) + colors[i1] * t


def color_ratio(ar_tex, pmdg_tex, colors, uv):
    """The SolidColor and the Mix ratio EveMaterial::scatter builds (eve.rs:98-111): ([N, 3], [N])."""
    ar = get_f(ar_tex, uv)
    pm = get_f(pmdg_tex, uv)
    albedo, roughness = ar[:, :3], ar[:, 3]
    paint, material, dirt = pm[:, 0:1], pm[:, 1], pm[:, 2] * ONE
    mc = palette(colors, material)
    d = dirt[:, None]
    color = (((albedo * mc * (ONE - paint)) + (albedo * paint)) * (ONE - np.fmin(d, ONE))) \
        + (_a([0.01, 0.005, 0.0]) * d)
    return color, np.fmin(roughness + dirt, ONE)


def emit(pmdg_tex, glow, uv):
    """EveMaterial::emit (eve.rs:121-128): glow_color * glow * 10.0"""
    g = get_f(pmdg_tex, uv)[:, 3:4]
    return _a(glow).reshape(1, 3) * g * f32(10.0)


def tangent_frame(a, b, c, uva, uvb, uvc):
    """Triangle::with_norms_and_uvs (geom.rs:474-482): (tangent, bitangent), [N, 3] each."""
    a, b, c, uva, uvb, uvc = map(_a, (a, b, c, uva, uvb, uvc))
    ab, ac = b - a, c - a
    uab, uac = uvb - uva, uvc - uva
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ONE / (uab[:, 0] * uac[:, 1] - uab[:, 1] * uac[:, 0])
    r = np.fmax(np.fmin(r, ONE), -ONE)[:, None]  # f32::min/max ignore a NaN operand
    with np.errstate(invalid="ignore"):
        tangent = (ab * uac[:, 1:2] - ac * uab[:, 1:2]) * r
        bitangent = (ac * uab[:, 0:1] - ab * uac[:, 0:1]) * r
    return tangent, bitangent


def triangle_hit(tri, ro, rd, t):
    """Triangle::intersect after the hit is accepted (geom.rs:535-552): the
    interpolated (normal, uv) at ray.at(t). tri: dict of [N, .] arrays a b c na nb nc uva uvb uvc."""
    point = ro + rd * t[:, None]
    d0, d1, d2 = tri["a"] - point, tri["b"] - point, tri["c"] - point
    area = length(cross(tri["a"] - tri["b"], tri["a"] - tri["c"]))
    a0 = (length(cross(d1, d2)) / area)[:, None]
    a1 = (length(cross(d2, d0)) / area)[:, None]
    a2 = (length(cross(d0, d1)) / area)[:, None]
    normal = tri["na"] * a0 + tri["nb"] * a1 + tri["nc"] * a2
    uv = tri["uva"] * a0 + tri["uvb"] * a1 + tri["uvc"] * a2
    return normal, uv


def mapped_normal(tangent, bitangent, normal, tan):
    """geom.rs:554-557: tangent * n.x + bitangent * n.y + normal * n.z"""
    return tangent * tan[:, 0:1] + bitangent * tan[:, 1:2] + normal * tan[:, 2:3]


def face_normal(rd, outward):
    """Hit::set_face_normal (geom.rs:17-24): (front_face [N] bool, normal [N, 3])."""
    front = dot(rd, outward) < 0
    return front, np.where(front[:, None], outward, -outward)


def instance_normal(fwd16, n):
    """Instance::intersect's way back (geom.rs:414-416): transform.transform_vector(normal).unit()"""
    return unit(transform(fwd16, n, 0.0))
