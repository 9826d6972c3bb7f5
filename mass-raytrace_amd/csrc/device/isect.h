// isect.h — a ray against one primitive or box: the division helpers, the ray
// of the space being traversed, the sphere, triangle and box tests, the
// triangle's shading record and alpha test, an instance's transform.
//   BoundingBox::hit      geom.rs:218-247
//   Sphere::intersect     geom.rs:56-93
//   Triangle::intersect   geom.rs:504-585 (candidate test; shading deferred)
//   Instance::intersect   geom.rs:403-420 (the ray's transform)
#pragma once
#include "../mrt_rng.h"
#include "surface.h"

namespace mrt {

// Correctly rounded quotient a/b from y = RN(1/b) (computed once per ray,
// rcp_cr: exactly the IEEE 1/b): q0 = a*y can be ~2 ulp off; one FMA residual
// correction makes it faithful and a second rounds it exactly (Markstein's
// theorem: y within 1/2 ulp of 1/b + faithful q => RN(q + (a - bq)y) = RN(a/b),
// absent under/overflow). Results outside [2^-90, 2^90], dividends below
// 2^-100 and divisors outside [2^-60, 2^60] take the plain division. 1 mul + 4 fma instead of the ~10
// instruction v_div_scale/v_rcp/v_div_fmas/v_div_fixup sequence; verified
// bit-exact against `a / b` by mrt_selftest_division.
struct Recip {
  float b, y;
};
MRT_HD Recip make_recip(float b) {
  Recip r;
  r.b = b;
  r.y = rcp_cr(b);
  return r;
}
// divisor inside the fast path's range
MRT_HD bool recip_ok(const Recip& r) { return fabsf(r.b) >= 0x1p-60f && fabsf(r.b) <= 0x1p60f; }
// q ~ RN(a/b) from y = RN(1/b): one product, two FMA residual corrections
MRT_HD float qfast(float a, float b, float y) {
  float q = a * y;
  float e = fmaf(-q, b, a);
  q = fmaf(e, y, q);
  e = fmaf(-q, b, a);
  return fmaf(e, y, q);
}
// exact whenever div_in_range(q, a) and the divisor was `ok`
MRT_HD float div_fast(float a, const Recip& r) { return qfast(a, r.b, r.y); }
// fast path valid: quotient in [2^-90, 2^90] and dividend >= 2^-100 (else the
// FMA residual a - q*b can fall into the subnormal range and lose bits)
MRT_HD bool div_in_range(float q, float a) {
  float aq = fabsf(q);
  return (aq <= 0x1p90f && aq >= 0x1p-90f && fabsf(a) >= 0x1p-100f) || a == 0.0f;
}
MRT_HD float div_cr(float a, const Recip& r) {
  float q = div_fast(a, r);
  if (!recip_ok(r) || !div_in_range(q, a)) q = a / r.b;
  return q;
}
// Ray in the space being traversed (world, or an instance's object space)
// with what the slab test needs: y = RN(1/d) per axis, the products
// oy = RN(o*y) of the early slab decision, its error margin om, and |d|^2.
struct TRay {
  V3 o, d;
  float yx, yy, yz;
  float oyx, oyy, oyz;  // RN(o.k * y.k)
  // |om| = max(max_k |oy.k| * 2^-20, 2^-120), the early decision's absolute
  // margin term (box_hit_any), or +inf when the early decision does not apply
  // to this ray (outside the early domain below: every box test is exact);
  // its sign bit set: the exact test may NOT use qfast (the ray or the scene
  // is outside the qfast domain below)
  float om;
  Recip a;  // |d|^2 for Sphere::intersect
};
// the early slab decision applies to this ray (early domain below)
MRT_HD bool tray_fast(const TRay& r) { return fabsf(r.om) != INFINITY; }
// qfast domain: with every box coordinate and ray-origin coordinate in
// {0} U [2^-40, 2^28] (scene bound checked on the host, origin here) each
// nonzero numerator (min - o) is >= 2^-63 and < 2^29; with |d| in
// [2^-20, 2^20] every quotient lies in [2^-83, 2^49] — inside div_fast's
// exact range — so no per-quotient check is needed.
// Early domain (slab_fast): its error bound needs no lower bound on the
// coordinates, only that no product overflows — box and origin coordinates
// finite and within 2^28, |d| in [2^-20, 2^20] — plus an absolute 2^-149 per
// rounding in the subnormal range, which the 2^-120 floor of |om| covers. (A
// mesh vertex at sin(pi) ~ 1e-16 is outside the qfast domain; until round 2's
// split it switched the whole 1M-triangle mesh_ply scene to the exact test.)
MRT_HD bool coord_ok(float c) {
  float a = fabsf(c);
  return a == 0.0f || (a >= 0x1p-40f && a <= 0x1p28f);
}
MRT_HD bool orig_ok(float c) { return fabsf(c) <= 0x1p28f; }
MRT_HD bool dir_ok(float c) {
  float a = fabsf(c);
  return a >= 0x1p-20f && a <= 0x1p20f;
}
// scene_flags (DevScene::fast_ok): bit 0 every box coordinate in the qfast
// domain, bit 1 every box coordinate finite and within 2^28.
MRT_HD TRay make_tray(V3 o, V3 d, uint32_t scene_flags) {
  TRay r;
  r.o = o;
  r.d = d;
  r.yx = rcp_cr(d.x);
  r.yy = rcp_cr(d.y);
  r.yz = rcp_cr(d.z);
  r.oyx = o.x * r.yx;
  r.oyy = o.y * r.yy;
  r.oyz = o.z * r.yz;
  const float om = fmaxf(fmaxf(fmaxf(fabsf(r.oyx), fabsf(r.oyy)), fabsf(r.oyz)) * 0x1p-20f, 0x1p-120f);
  r.a = make_recip(length_squared(d));
  const bool dok = dir_ok(d.x) && dir_ok(d.y) && dir_ok(d.z);
  const bool qok = (scene_flags & 1u) && coord_ok(o.x) && coord_ok(o.y) && coord_ok(o.z) && dok;
  const bool fast = (scene_flags & 2u) && orig_ok(o.x) && orig_ok(o.y) && orig_ok(o.z) && dok;
  const float m = fast ? om : INFINITY;
  r.om = qok ? m : -m;
  return r;
}

// A NaN t's bits as the oracle's host computes them. The reference's range
// checks are false on NaN, so a t that is NaN is a hit and its bits are
// output (far origins: half_b^2 - a*c = inf - inf; a NaN in the ray). The
// device's instructions need not give the host's NaN: where an operation
// makes one out of numbers (inf - inf, 0 * inf) v_add / v_mul give 0x7FC00000
// and the host (x86 SSE) 0xFFC00000, and a NaN operand is not always passed
// on with the host's sign (seen on the MI355X after the square root and the
// division, and in the triangle test). Which NaN the walk carries changes no
// comparison, so the walk is left alone (k_trace sits at its register cap)
// and mrt_trace_rays' output kernel (trace.hip k_rays_out) computes the
// winner's expression again where its t is NaN, operation for operation, with
// every NaN result chosen by the host's rule: the first operand if it is NaN,
// else the second, else the default NaN 0xFFC00000. Operands in the order of
// the oracle's source; that this gives the oracle's bits is checked on every
// NaN t of the adversarial families (tests/test_gpu_adversarial.py).
// Sphere: the first root if it is NaN (every check on it is false: accepted
// at once), else the second (the first was a number, and was refused).
MRT_HD float host_nan(float res, float x, float y) {
  return x != x ? x : y != y ? y : res != res ? u2f(0xFFC00000u) : res;
}
MRT_HD float hn_sub(float x, float y) { return host_nan(x - y, x, y); }
MRT_HD float hn_add(float x, float y) { return host_nan(x + y, x, y); }
MRT_HD float hn_mul(float x, float y) { return host_nan(x * y, x, y); }
MRT_HD float hn_div(float x, float y) { return host_nan(x / y, x, y); }
MRT_HD float hn_dot(V3 x, V3 y) { return hn_add(hn_add(hn_mul(x.x, y.x), hn_mul(x.y, y.y)), hn_mul(x.z, y.z)); }
MRT_HD V3 hn_cross(V3 x, V3 y) {
  return V3{hn_sub(hn_mul(x.y, y.z), hn_mul(x.z, y.y)), hn_sub(hn_mul(x.z, y.x), hn_mul(x.x, y.z)),
            hn_sub(hn_mul(x.x, y.y), hn_mul(x.y, y.x))};
}
MRT_HD float sphere_root_nan(V3 c, float r, V3 o, V3 d) {
  const float a = hn_dot(d, d);
  const V3 oc{hn_sub(o.x, c.x), hn_sub(o.y, c.y), hn_sub(o.z, c.z)};
  const float half_b = hn_dot(oc, d);
  const float cc = hn_sub(hn_dot(oc, oc), hn_mul(r, r));
  const float disc = hn_sub(hn_mul(half_b, half_b), hn_mul(a, cc));
  const float sq = disc != disc ? disc : sqrtf(disc);
  const float first = hn_div(hn_sub(-half_b, sq), a);
  return first != first ? first : hn_div(hn_add(-half_b, sq), a);
}
// the same for a triangle's t (Triangle::intersect's expression, tri_hit) and
// for the ray an instance's inverse makes (xform)
MRT_HD float tri_t_nan(V3 a, V3 ab, V3 ac, V3 o, V3 d) {
  const float inv_det = hn_div(1.0f, hn_dot(ab, hn_cross(d, ac)));
  const V3 t_vec{hn_sub(o.x, a.x), hn_sub(o.y, a.y), hn_sub(o.z, a.z)};
  return hn_mul(hn_dot(ac, hn_cross(t_vec, ab)), inv_det);
}
MRT_HD V3 xform_nan(V3 c0, V3 c1, V3 c2, V3 c3, V3 p, float w) {
  auto row = [&](float k0, float k1, float k2, float k3) {
    return hn_add(hn_add(hn_add(hn_mul(k0, p.x), hn_mul(k1, p.y)), hn_mul(k2, p.z)), hn_mul(k3, w));
  };
  return V3{row(c0.x, c1.x, c2.x, c3.x), row(c0.y, c1.y, c2.y, c3.y), row(c0.z, c1.z, c2.z, c3.z)};
}

MRT_HD bool sphere_hit(V3 c, float r, V3 o, V3 d, const Recip& ra, float tmin, float tmax, float& t) {
  V3 oc = o - c;
  float a = ra.b;  // length_squared(d), precomputed per ray
  float half_b = dot(oc, d);
  float cc = length_squared(oc) - (r * r);
  float disc = (half_b * half_b) - (a * cc);
  if (disc < 0.0f) return false;
  float sq = sqrtf(disc);
  float root = div_cr(-half_b - sq, ra);
  if (root < tmin || tmax < root) {
    root = div_cr(-half_b + sq, ra);
    if (root < tmin || tmax < root) return false;
  }
  t = root;
  return true;
}

MRT_HD bool tri_hit(V3 a, V3 ab, V3 ac, V3 o, V3 d, float tmin, float tmax, float& t) {
  V3 p_vec = cross(d, ac);
  float det = dot(ab, p_vec);
  if (fabsf(det) < 0.000001f) return false;
  float inv_det = rcp_cr(det);  // RN(1 / det), as the reference's 1.0 / det
  V3 t_vec = o - a;
  float u = dot(t_vec, p_vec) * inv_det;
  if (u < 0.0f || u > 1.0f) return false;
  V3 q_vec = cross(t_vec, ab);
  float v = dot(d, q_vec) * inv_det;
  if (v < 0.0f || v + u > 1.0f) return false;
  float tt = dot(ac, q_vec) * inv_det;
  if (tt < tmin || tt > tmax) return false;
  t = tt;
  return true;
}

// The same test without early exits (the near-first leaf step, whose lanes
// are mixed: every lane pays the whole test either way, and the exits cost
// exec-mask juggling): identical arithmetic, the conditions combined at the end.
MRT_HD bool tri_hit_nb(V3 a, V3 ab, V3 ac, V3 o, V3 d, float tmin, float tmax, float& t) {
  V3 p_vec = cross(d, ac);
  float det = dot(ab, p_vec);
  float inv_det = rcp_cr(det);
  V3 t_vec = o - a;
  float u = dot(t_vec, p_vec) * inv_det;
  V3 q_vec = cross(t_vec, ab);
  float v = dot(d, q_vec) * inv_det;
  float tt = dot(ac, q_vec) * inv_det;
  t = tt;
  return !(fabsf(det) < 0.000001f) && !(u < 0.0f || u > 1.0f) && !(v < 0.0f || v + u > 1.0f) && !(tt < tmin || tt > tmax);
}

struct TriShade {
  V3 a, b, c, na, nb, nc;
  V2 uva, uvb, uvc;
  uint32_t material, flags;
  uint32_t eve;  // TRI_FLAG_EVE: the Eve record of the triangle's own material
};
MRT_HD TriShade load_tri(const DevScene& S, uint32_t id) {
  const float4* q = reinterpret_cast<const float4*>(S.tri_shade) + (size_t)MRT_IDX(S, id, S.n_tris, 3) * kTriShadeQuads;
  float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6];
  TriShade s;
  s.a = V3{q0.x, q0.y, q0.z};
  s.b = V3{q0.w, q1.x, q1.y};
  s.c = V3{q1.z, q1.w, q2.x};
  s.na = V3{q2.y, q2.z, q2.w};
  s.nb = V3{q3.x, q3.y, q3.z};
  s.nc = V3{q3.w, q4.x, q4.y};
  s.uva = V2{q4.z, q4.w};
  s.uvb = V2{q5.x, q5.y};
  s.uvc = V2{q5.z, q5.w};
  s.material = f2u(q6.x);
  s.flags = f2u(q6.y);
  s.eve = f2u(q6.z);
  return s;
}

// Area-ratio barycentrics of the accepted point (geom.rs:535-547)
MRT_HD void tri_bary(const TriShade& s, V3 point, float& a0, float& a1, float& a2) {
  V3 d0 = s.a - point, d1 = s.b - point, d2 = s.c - point;
  float area = length(cross(s.a - s.b, s.a - s.c));
  a0 = length(cross(d1, d2)) / area;
  a1 = length(cross(d2, d0)) / area;
  a2 = length(cross(d0, d1)) / area;
}

// Material::alpha_test of the triangle's OWN material (geom.rs:567-571,
// material.rs:222-224,281-283): surface alpha != 0.
template <bool RNG, bool EXT>
MRT_HD bool tri_alpha_pass(const DevScene& S, uint32_t id, V3 o, V3 d, float t, PathRng& rng, LocalCounters& lc) {
  TriShade s = load_tri(S, id);
  V3 point = o + d * t;
  float a0, a1, a2;
  tri_bary(s, point, a0, a1, a2);
  V2 uv = (s.uva * a0 + s.uvb * a1) + s.uvc * a2;
  GpuMaterial m = S.materials[MRT_IDX(S, s.material, S.n_materials, 4)];
  // Mix::alpha_test draws to pick a side (material.rs:418-424)
  if (RNG)
    while (m.kind == MRT_MAT_MIX) m = S.materials[MRT_IDX(S, rng.f32() < m.param ? m.left : m.right, S.n_materials, 4)];
  // Lambertian/Metal alpha_test; Specular's forwards to its inner Lambertian
  if (m.kind != MRT_MAT_LAMBERTIAN && m.kind != MRT_MAT_METAL && m.kind != MRT_MAT_SPECULAR) return true;
  return surface_get_f<EXT>(S, m, uv, lc).w != 0.0f;
}

MRT_HD void load_m12(const float* p, V3& c0, V3& c1, V3& c2, V3& c3) {
  c0 = V3{p[0], p[1], p[2]};
  c1 = V3{p[3], p[4], p[5]};
  c2 = V3{p[6], p[7], p[8]};
  c3 = V3{p[9], p[10], p[11]};
}
// M4::transform (generic.rs:106-115) on the xyz rows: ((c0*x + c1*y) + c2*z) + c3*w
MRT_HD V3 xform(V3 c0, V3 c1, V3 c2, V3 c3, V3 p, float w) {
  return ((c0 * p.x + c1 * p.y) + c2 * p.z) + c3 * w;
}

// f32 min/max without the canonicalising v_max hipcc inserts before fminf:
// every operand here is an arithmetic result (never a signalling NaN), for
// which v_min/v_max/v_min3/v_max3 are IEEE minNum/maxNum = Rust f32::min/max
// (= the host's fminf/fmaxf).
#if defined(__HIP_DEVICE_COMPILE__)
MRT_HD float vmin1(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
MRT_HD float vmax1(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
MRT_HD float vmin3(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
MRT_HD float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// max(|a|, |b|, c) in one instruction (the abs as source modifiers)
MRT_HD float vmax3ab(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
#else
MRT_HD float vmin1(float a, float b) { return fminf(a, b); }
MRT_HD float vmax1(float a, float b) { return fmaxf(a, b); }
MRT_HD float vmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
MRT_HD float vmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
MRT_HD float vmax3ab(float a, float b, float c) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), c); }
#endif

// BoundingBox::hit (geom.rs:218-247): v_min = (min - o)/d, v_max = (max - o)/d,
// six correctly rounded quotients — qfast in the ray's fast domain (bit-identical
// to IEEE division there), IEEE division otherwise. The per-axis early-outs
// cannot change the result (t0 only grows, t1 only shrinks, NaNs are ignored
// by min/max): one final compare of max(tmin, lo) against min(tmax, hi).
MRT_HD bool box_hit_exact(V3 mn, V3 mx, const TRay& r, float tmin, float tmax) {
  V3 na = mn - r.o, nb = mx - r.o;
  V3 a{qfast(na.x, r.d.x, r.yx), qfast(na.y, r.d.y, r.yy), qfast(na.z, r.d.z, r.yz)};
  V3 b{qfast(nb.x, r.d.x, r.yx), qfast(nb.y, r.d.y, r.yy), qfast(nb.z, r.d.z, r.yz)};
  if (signbit(r.om)) {  // outside the qfast domain
    a = na / r.d;
    b = nb / r.d;
  }
  float t0 = vmax3(vmin1(a.x, b.x), vmin1(a.y, b.y), vmax1(vmin1(a.z, b.z), tmin));
  float t1 = vmin3(vmax1(a.x, b.x), vmax1(a.y, b.y), vmin1(vmax1(a.z, b.z), tmax));
  return !(t1 < t0);
}

// The same decision, cheaper: in the fast domain a = RN(m*y - RN(o*y)) (one
// FMA per slab plane) is within |Q|*2^-22.4 + |o*y|*2^-23.9 of the correctly
// rounded quotient RN((m - o)/d) — one rounding in y = RN(1/d), one in o*y,
// one in the FMA, half an ulp to the quotient; no under/overflow in the fast
// domain. min/max are 1-Lipschitz and the terms that decide them lie at t0
// (t1), so t0 and t1 carry that bound relative to their own magnitude plus
// max_k |o.k*y.k|*2^-23.9. When t1 - t0 exceeds (|t0|+|t1|)*2^-19 + |om| (|om| >=
// max_k |o.k*y.k|*2^-20, 4x slack on both terms) the comparison of the exact
// values is decided; otherwise — grazing rays, flat boxes, ties — the exact
// test decides. mrt_selftest_slab checks this against box_hit_exact on
// near-tie boxes.
MRT_HD void slab_fast(V3 mn, V3 mx, const TRay& r, float tmin, float tmax, float& t0, float& t1) {
  const float ax = fmaf(mn.x, r.yx, -r.oyx), ay = fmaf(mn.y, r.yy, -r.oyy), az = fmaf(mn.z, r.yz, -r.oyz);
  const float bx = fmaf(mx.x, r.yx, -r.oyx), by = fmaf(mx.y, r.yy, -r.oyy), bz = fmaf(mx.z, r.yz, -r.oyz);
  t0 = vmax3(vmin1(ax, bx), vmin1(ay, by), vmax1(vmin1(az, bz), tmin));
  t1 = vmin3(vmax1(ax, bx), vmax1(ay, by), vmin1(vmax1(az, bz), tmax));
}
MRT_HD float slab_margin(const TRay& r, float t0, float t1) {
  return fmaf(fabsf(t0) + fabsf(t1), 0x1p-19f, fabsf(r.om));
}
template <bool COUNT = false>
MRT_HD bool box_hit_any(V3 mn, V3 mx, const TRay& r, float tmin, float tmax, LocalCounters* lc = nullptr) {
  // no branch on the ray's domain: outside the early domain |om| = +inf makes
  // the margin +inf (or NaN), so neither comparison decides and the exact
  // test runs
  {
    float t0, t1;
    slab_fast(mn, mx, r, tmin, tmax, t0, t1);
    const float m = slab_margin(r, t0, t1);
    const float gap = t1 - t0;
    if (gap > m) return true;
    if (-gap > m) return false;
  }
  if (COUNT) lc->box_exact++;
  return box_hit_exact(mn, mx, r, tmin, tmax);
}

}  // namespace mrt
