// material.h — from the closest hit to the next ray: the hit record, sampling,
// the camera, backgrounds, scattering.
//   Camera::ray           world.rs:53-63
//   Material::scatter/emit material.rs:203-329,385-389
//   Background            material.rs:49-89
#pragma once
#include "walk.h"

namespace mrt {

// Hit record of the closest hit, computed the way the reference's winning
// intersect computed it (geom.rs:77-91,535-584,405-419,318-326).
struct Surf {
  V3 point, normal;
  V2 uv;
  bool has_uv, front_face;
  uint32_t material;
};

// A loaded value pinned where it was loaded: the compiler otherwise sinks a
// load to the block of its first use, behind the waits in between (a
// sphere's material index went out only after its centre had arrived and the
// normal's divisions had run). Generates no instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define MRT_PIN_LOAD(x) asm volatile("" : "+v"(x))
#else
#define MRT_PIN_LOAD(x) (void)0
#endif

// An EveMaterial record (layout.h kEveQuads): its texture indices.
struct EveTex {
  uint32_t normal_occlusion, albedo_roughness, pmdg;
};
MRT_HD const float* eve_record(const DevScene& S, uint32_t rec) {
  return S.eve + (size_t)MRT_IDX(S, rec, S.n_eve, 25) * (kEveQuads * 4);
}
MRT_HD EveTex load_eve_tex(const DevScene& S, uint32_t rec) {
  const float4 q = *reinterpret_cast<const float4*>(eve_record(S, rec));
  return EveTex{f2u(q.x), f2u(q.y), f2u(q.z)};
}
// EveMaterial::normal_occlusion (eve.rs:66-73): the tangent-space normal
MRT_HD V3 eve_tangent_normal(const DevScene& S, uint32_t rec, V2 uv, LocalCounters& lc) {
  const V4 px = texture_get_f(S, load_eve_tex(S, rec).normal_occlusion, uv, lc);
  const float py = px.y * 2.0f - 1.0f, pw = px.w * 2.0f - 1.0f;
  const float x = (1.0f - py * py) - pw * pw;
  return unit(V3{py, pw, sqrtf(fabsf(x))});
}

// EXT: the scene may hold EveMaterial triangles, whose normal is mapped
// (Material::normal, geom.rs:551-560); lc counts the normal map's taps.
template <bool EXT>
MRT_HD Surf resolve_hit(const DevScene& S, V3 o, V3 d, const Hit& h, LocalCounters& lc) {
  Surf s;
  V3 ro = o, rd = d;
  const uint32_t ckind = h.container >> 28, cidx = h.container & 0x0FFFFFFFu;
  V3 f0, f1, f2, f3;
  // the container's override material goes out with the first gather of the
  // hit (the instance's inverse, the triangle's quads), not behind the last.
  // (inst_fwd stays behind the barycentrics: held through them, its 12
  // registers put 24 B of k_shade's 7-waves variant into scratch.)
  uint32_t over = MRT_NO_MATERIAL;
  if (ckind == MRT_REF_INSTANCE) {
    V3 c0, c1, c2, c3;
    over = S.inst_mat[MRT_IDX(S, cidx, S.n_inst, 12)];
    load_m12(S.inst_inv + (size_t)MRT_IDX(S, cidx, S.n_inst, 9) * 12, c0, c1, c2, c3);
    ro = xform(c0, c1, c2, c3, o, 1.0f);
    rd = xform(c0, c1, c2, c3, d, 0.0f);
  } else if (ckind == MRT_REF_MODEL) {
    over = S.model_mat[MRT_IDX(S, cidx, S.n_models, 13)];
  }
  const uint32_t pkind = h.prim >> 28, pidx = h.prim & 0x0FFFFFFFu;
  V3 outward;
  s.point = ro + rd * h.t;
  if (pkind == MRT_REF_VOLUME) {  // geom.rs:644-651: fixed normal, front face, no uv
    s.normal = V3{1.0f, 0.0f, 0.0f};
    s.front_face = true;
    s.has_uv = false;
    s.uv = V2{0, 0};
    s.material = S.vol_mat[MRT_IDX(S, pidx, S.n_vol, 16)];
    return s;  // volumes are World objects: no container
  }
  if (pkind == MRT_REF_SPHERE) {
    const uint32_t sp = MRT_IDX(S, pidx, S.n_sph, 10);
    V3 c = ld3(S.sph + (size_t)sp * 4);
    float r = S.sph[(size_t)sp * 4 + 3];
    s.material = S.sph_mat[sp];  // with {c, r}: one wait for both
    MRT_PIN_LOAD(s.material);
    outward = (s.point - c) / r;
    s.has_uv = false;
    s.uv = V2{0, 0};
  } else {
    TriShade t = load_tri(S, pidx);
    // the tangent frame with the triangle's other quads (a scene without an
    // Eve material has none: a uniform branch)
    float4 tq{}, bq{};
    if (EXT && S.tri_tb) {
      const float4* tb = reinterpret_cast<const float4*>(S.tri_tb) + (size_t)MRT_IDX(S, pidx, S.n_tris, 3) * 2;
      tq = tb[0], bq = tb[1];
    }
    float a0, a1, a2;
    tri_bary(t, s.point, a0, a1, a2);
    outward = (t.na * a0 + t.nb * a1) + t.nc * a2;
    s.has_uv = (t.flags & TRI_FLAG_UV) != 0;
    s.uv = uv_or_zero(s.has_uv, (t.uva * a0 + t.uvb * a1) + t.uvc * a2);
    s.material = t.material;
    // the triangle's OWN material's normal map (geom.rs:554), whatever override follows
    if (EXT && S.tri_tb && s.has_uv && (t.flags & TRI_FLAG_EVE)) {
      const V3 tn = eve_tangent_normal(S, t.eve, s.uv, lc);
      outward = ((V3{tq.x, tq.y, tq.z} * tn.x) + (V3{bq.x, bq.y, bq.z} * tn.y)) + (outward * tn.z);
    }
  }
  // Hit::set_face_normal in the intersecting (object) space (geom.rs:17-24)
  s.front_face = dot(rd, outward) < 0.0f;
  s.normal = s.front_face ? outward : -outward;
  if (ckind == MRT_REF_INSTANCE) {
    load_m12(S.inst_fwd + (size_t)MRT_IDX(S, cidx, S.n_inst, 11) * 12, f0, f1, f2, f3);
    s.point = xform(f0, f1, f2, f3, s.point, 1.0f);
    s.normal = unit(xform(f0, f1, f2, f3, s.normal, 0.0f));
  }
  if (over != MRT_NO_MATERIAL) s.material = over;
  return s;
}
// scenes without an Eve material (the non-EXT kernels, the host checks)
MRT_HD Surf resolve_hit(const DevScene& S, V3 o, V3 d, const Hit& h) {
  LocalCounters lc;
  return resolve_hit<false>(S, o, d, h, lc);
}

// ---- sampling (math.rs:262-291) -----------------------------------------------
MRT_DEV V3 random_in_unit_sphere(PathRng& rng) {
  for (;;) {
    float x = rng.f32() * 2.0f - 1.0f;
    float y = rng.f32() * 2.0f - 1.0f;
    float z = rng.f32() * 2.0f - 1.0f;
    V3 v{x, y, z};
    if (length_squared(v) >= 1.0f) continue;
    return v;
  }
}
MRT_DEV V3 random_in_unit_disk(PathRng& rng) {
  for (;;) {
    float x = rng.f32() * 2.0f - 1.0f;
    float y = rng.f32() * 2.0f - 1.0f;
    V3 v{x, y, 0.0f};
    if (length_squared(v) >= 1.0f) continue;
    return v;
  }
}

// Dielectric::reflectance (material.rs:296-299); powi(5) = x*((x*x)*(x*x))
MRT_DEV float reflectance(float cosine, float ref_idx) {
  float r0 = (1.0f - ref_idx) / (1.0f + ref_idx);
  r0 = r0 * r0;
  float x = 1.0f - cosine;
  return r0 + (1.0f - r0) * (x * ((x * x) * (x * x)));
}

struct DevCamera {
  V3 origin, llc, horizontal, vertical, u, v;
  float lens_radius;
};

// main.rs:258-260 + Camera::ray (world.rs:53-63)
// Camera::ray (world.rs:53-63) through (u, v)
MRT_DEV void camera_ray_uv(const DevCamera& cam, float u, float v, PathRng& rng, V3& o, V3& d) {
  V3 blur = random_in_unit_disk(rng) * cam.lens_radius;
  V3 offset = cam.u * blur.x + cam.v * blur.y;
  o = cam.origin + offset;
  d = (((cam.llc + (cam.horizontal * u)) + (cam.vertical * v)) - cam.origin) - offset;
}

// the jittered sample ray of pixel (x, y) (main.rs:258-260)
MRT_DEV void camera_ray(const DevCamera& cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H, PathRng& rng, V3& o,
                        V3& d) {
  float u = ((float)x + rng.f32()) / (float)(W - 1);
  float v = ((float)y + rng.f32()) / (float)(H - 1);
  camera_ray_uv(cam, u, v, rng, o, d);
}

template <bool EXT>
MRT_DEV V3 background(const DevScene& S, V3 d, LocalCounters& lc) {
  if (S.bg_kind == MRT_BG_SOLID) return V3{S.bg_color[0], S.bg_color[1], S.bg_color[2]};
  if (S.bg_kind == MRT_BG_SKY) {
    V3 ud = unit(d);
    float t = 0.5f * (ud.y + 1.0f);
    return (fill3(1.0f) * (1.0f - t)) + (V3{0.5f, 0.7f, 1.0f} * t);
  }
  V2 uv{0.0f, 0.0f};
  uint32_t face = 0;
  if (!EXT || S.bg_kind == MRT_BG_SKYSPHERE) {
    V3 p = unit(d);
    float theta = acosf(p.y);
    float phi = atan2f(p.z * -1.0f, p.x) + kPi;
    uv = V2{phi / (2.0f * kPi), theta / kPi};
  } else if (EXT) {  // CubeMap::background (material.rs:122-189); y faces swapped as in the reference
    const float* mf = S.bg_m;
    const M4 m{V4{mf[0], mf[1], mf[2], mf[3]}, V4{mf[4], mf[5], mf[6], mf[7]}, V4{mf[8], mf[9], mf[10], mf[11]},
               V4{mf[12], mf[13], mf[14], mf[15]}};
    V3 p = transform(m, d, 0.0f);
    V3 a{fabsf(p.x), fabsf(p.y), fabsf(p.z)};
    float max_axis = 0.0f, u = 0.0f, v = 0.0f;
    if (a.x >= a.y && a.x >= a.z) {
      if (p.x > 0.0f) face = 0, u = p.z * -1.0f, v = p.y;
      else face = 1, u = p.z, v = p.y;
      max_axis = a.x;
    } else if (a.y >= a.x && a.y >= a.z) {
      if (p.y > 0.0f) face = 3, u = p.x, v = p.z * -1.0f;
      else face = 2, u = p.x, v = p.z;
      max_axis = a.y;
    } else if (a.z >= a.x && a.z >= a.y) {
      if (p.z > 0.0f) face = 4, u = p.x, v = p.y;
      else face = 5, u = p.x * -1.0f, v = p.y;
      max_axis = a.z;
    }
    uv = V2{0.5f * (u / max_axis + 1.0f), 0.5f * (v / max_axis + 1.0f)};
  }
  const GpuSurfRef f = S.bg_faces[face];
  V4 px = surface_ref_get_f<EXT>(S, f.kind, f.index, f.len, f.color, uv, lc);
  return V3{px.x, px.y, px.z};
}

// Hit::emit + Hit::scatter (geom.rs:26-32). Returns true when the path
// continues with (new_o, new_d) and attenuation `atten`.
//
// The head of a material record, q0 and q1 of GpuMaterial (layout.h): what
// every kind reads, two 16-B loads issued together. q2 (left, right,
// surf_len) is read only where a Mix or a composite surface needs it.
struct MatHead {
  uint32_t kind, surf_kind, texture;
  float param;
  float color[4];
};
MRT_DEV MatHead load_mat_head(const DevScene& S, uint32_t mi) {
  const GpuMaterial* p = S.materials + MRT_IDX(S, mi, S.n_materials, 4);
  return MatHead{p->kind, p->surf_kind, p->texture, p->param, {p->color[0], p->color[1], p->color[2], p->color[3]}};
}
// Mix::scatter/emit/alpha_test (material.rs:402-424): every call draws once
// to pick a side, recursively; children precede their Mix in the table.
// `m` is the head of record `mi` (the caller's register copy of the hit's
// root record): a material that is no Mix draws nothing and loads nothing.
// Returns the picked record's index, its head in `m`.
MRT_DEV uint32_t mix_pick(const DevScene& S, uint32_t mi, MatHead& m, PathRng& rng) {
  while (m.kind == MRT_MAT_MIX) {
    const GpuMaterial* p = S.materials + MRT_IDX(S, mi, S.n_materials, 4);
    const uint32_t left = p->left, right = p->right;
    mi = rng.f32() < m.param ? left : right;
    m = load_mat_head(S, mi);
  }
  return mi;
}
template <bool EXT>
MRT_DEV V4 mat_get_f(const DevScene& S, const MatHead& m, uint32_t mi, V2 uv, LocalCounters& lc) {
  uint32_t len = 0;
  if (EXT && m.surf_kind == SURF_PROGRAM) len = S.materials[MRT_IDX(S, mi, S.n_materials, 4)].surf_len;
  return surface_ref_get_f<EXT>(S, m.surf_kind, m.texture, len, m.color, uv, lc);
}

// Lambertian::scatter (material.rs:203-215)
template <bool EXT>
MRT_DEV void lambertian(const DevScene& S, const MatHead& m, uint32_t mi, const Surf& s, PathRng& rng, V3& atten,
                        V3& new_d, LocalCounters& lc) {
  V3 dir = s.normal + unit(random_in_unit_sphere(rng));
  if (near_zero(dir)) dir = s.normal;
  V4 c = mat_get_f<EXT>(S, m, mi, uv_or_zero(s.has_uv, s.uv), lc);
  atten = V3{c.x, c.y, c.z};
  new_d = dir;
}

// Hit::emit then Hit::scatter (world.rs:69-70), in that order of RNG draws.
// The hit's root record is fetched once; the emit pick and the scatter pick
// both start from that copy. root_kind: its kind (k_shade's survivor key).
template <bool EXT>
MRT_DEV bool scatter(const DevScene& S, const Surf& s, V3 d, PathRng& rng, V3& emitted, V3& atten, V3& new_d,
                     LocalCounters& lc, uint32_t& root_kind) {
  const MatHead root = load_mat_head(S, s.material);
  root_kind = root.kind;
  emitted = V3{0, 0, 0};
  // EveMaterial: the paint/material/dirt/glow texel of the record emit picked,
  // kept for scatter (the same record unless a Mix picked another)
  uint32_t pmdg_rec = 0xFFFFFFFFu;
  V4 pmdg{};
  {
    MatHead e = root;
    mix_pick(S, s.material, e, rng);
    if (e.kind == MRT_MAT_DIFFUSE_LIGHT) emitted = V3{e.color[0], e.color[1], e.color[2]};
    if (EXT && e.kind == MRT_MAT_EVE && s.has_uv) {  // eve.rs:121-128
      pmdg_rec = e.texture;
      pmdg = texture_get_f(S, load_eve_tex(S, pmdg_rec).pmdg, s.uv, lc);
      const float* g = eve_record(S, pmdg_rec) + 16;
      emitted = (V3{g[0], g[1], g[2]} * pmdg.w) * 10.0f;
    }
  }
  MatHead m = root;
  const uint32_t mi = mix_pick(S, s.material, m, rng);
  V2 uv = uv_or_zero(s.has_uv, s.uv);
  if (EXT && m.kind == MRT_MAT_EVE) {  // EveMaterial::scatter (eve.rs:92-119)
    if (!s.has_uv) return false;
    const uint32_t rec = m.texture;
    const EveTex tex = load_eve_tex(S, rec);
    const V4 ar = texture_get_f(S, tex.albedo_roughness, s.uv, lc);
    if (rec != pmdg_rec) pmdg = texture_get_f(S, tex.pmdg, s.uv, lc);
    const V3 albedo{ar.x, ar.y, ar.z};
    const float roughness = ar.w, paint = pmdg.x, dirt = pmdg.z;
    // EveMaterialColor::get (eve.rs:190-198); the reference would panic past colors[3]
    const float i = pmdg.y * 3.0f;
    uint32_t i0 = f2usize(floorf(i)), i1 = f2usize(ceilf(i));
    i0 = i0 < 3u ? i0 : 3u;
    i1 = i1 < 3u ? i1 : 3u;
    const float t = i - (float)i0;
    const float* pal = eve_record(S, rec) + 4;
    const V3 mc = (ld3(pal + 3 * i0) * (1.0f - t)) + (ld3(pal + 3 * i1) * t);
    const V3 color = ((((albedo * mc) * (1.0f - paint)) + (albedo * paint)) * (1.0f - fminf(dirt, 1.0f))) +
                     (V3{0.01f, 0.005f, 0.0f} * dirt);
    // Mix::new(ratio, Lambertian::new(color), Specular::new(1.8, color)).scatter: one draw
    // picks the side, which then runs below as any Lambertian or Specular over a SolidColor
    const float ratio = fminf(roughness + dirt, 1.0f);
    m = MatHead{rng.f32() < ratio ? MRT_MAT_LAMBERTIAN : MRT_MAT_SPECULAR, MRT_SURF_SOLID, 0u, 1.8f,
                {color.x, color.y, color.z, 1.0f}};
  }
  switch (m.kind) {
    case MRT_MAT_LAMBERTIAN:
      lambertian<EXT>(S, m, mi, s, rng, atten, new_d, lc);
      return true;
    case MRT_MAT_METAL: {
      V3 reflected = reflect(unit(d), s.normal);
      V3 dir = reflected + (random_in_unit_sphere(rng) * m.param);
      if (dot(dir, s.normal) > 0.0f) {
        V4 c = mat_get_f<EXT>(S, m, mi, uv, lc);
        atten = V3{c.x, c.y, c.z};
        new_d = dir;
        return true;
      }
      return false;
    }
    case MRT_MAT_DIELECTRIC:
    case MRT_MAT_SPECULAR: {  // material.rs:299-328 / 355-377
      float ratio = s.front_face ? 1.0f / m.param : m.param;
      V3 ud = unit(d);
      float cos_theta = fminf(dot(-ud, s.normal), 1.0f);
      float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
      bool cannot_refract = ratio * sin_theta > 1.0f;
      if (cannot_refract || reflectance(cos_theta, ratio) > rng.f32()) {
        new_d = reflect(ud, s.normal);
      } else if (m.kind == MRT_MAT_SPECULAR) {
        lambertian<EXT>(S, m, mi, s, rng, atten, new_d, lc);  // return self.inner.scatter(ray, hit)
        return true;
      } else {
        new_d = refract(ud, s.normal, ratio);
      }
      atten = fill3(1.0f);
      return true;
    }
    case MRT_MAT_ISOTROPHIC:  // material.rs:438-444: direction not normalised
      atten = V3{m.color[0], m.color[1], m.color[2]};
      new_d = random_in_unit_sphere(rng);
      return true;
    default:  // DiffuseLight, ()
      return false;
  }
}

}  // namespace mrt
