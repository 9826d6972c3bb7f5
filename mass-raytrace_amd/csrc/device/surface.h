// surface.h — what a surface returns at (u, v): texels, the bilinear tap,
// composite surface programs.
//   Texture::get_f        texture.rs:126-148, WrapMode::wrap texture.rs:278-299
#pragma once
#include "devbase.h"

namespace mrt {

// ---- textures -----------------------------------------------------------
MRT_HD float rust_fract(float x) { return x - truncf(x); }
// `f32 as usize` saturates: NaN and negatives -> 0
MRT_HD uint32_t f2usize(float f) { return f > 0.0f ? (f < 4294967040.0f ? (uint32_t)f : 0xFFFFFFFFu) : 0u; }

MRT_HD V4 texel(const DevScene& S, const GpuTexture& t, uint32_t x, uint32_t y) {
  const uint32_t tpr = (t.width + kTexBlockW - 1) / kTexBlockW;  // layout.h: 8x4-texel blocks
  uint32_t v = S.texels[MRT_IDX(S, t.offset + texel_index(tpr, x, y), S.n_texels, 1)];
  return V4{(float)(v & 255u) / 255.0f, (float)((v >> 8) & 255u) / 255.0f, (float)((v >> 16) & 255u) / 255.0f,
            (float)(v >> 24) / 255.0f};
}

MRT_HD V4 texture_get_f(const DevScene& S, uint32_t tex, V2 uv, LocalCounters& lc) {
  const GpuTexture t = S.textures[MRT_IDX(S, tex, S.n_textures, 2)];
  float x = uv.x, y = uv.y;
  if (t.wrap == MRT_WRAP_REPEAT) {
    x = x < 0.0f ? 1.0f - rust_fract(fabsf(x)) : x;
    y = y < 0.0f ? 1.0f - rust_fract(fabsf(y)) : y;
    x = x > 1.0f ? rust_fract(x) : x;
    y = y > 1.0f ? rust_fract(y) : y;
  } else {
    x = fmaxf(fminf(x, 1.0f), 0.0f);
    y = fmaxf(fminf(y, 1.0f), 0.0f);
  }
  x = x * (float)(t.width - 1);
  y = y * (float)(t.height - 1);
  uint32_t x0 = f2usize(floorf(x)), x1 = f2usize(ceilf(x));
  uint32_t y0 = f2usize(floorf(y)), y1 = f2usize(ceilf(y));
  x0 = x0 < t.width ? x0 : t.width - 1;  // the reference would panic out of range
  x1 = x1 < t.width ? x1 : t.width - 1;
  y0 = y0 < t.height ? y0 : t.height - 1;
  y1 = y1 < t.height ? y1 : t.height - 1;
  float tt = x - (float)x0;
  V4 p0 = texel(S, t, x0, y0) * (1.0f - tt) + texel(S, t, x1, y0) * tt;
  V4 p1 = texel(S, t, x0, y1) * (1.0f - tt) + texel(S, t, x1, y1) * tt;
  tt = y - (float)y0;
  lc.texel_taps += 4;
  return p1 * tt + p0 * (1.0f - tt);
}

// YCbCrTexture::get_f tail (texture.rs:233-249): YUV_TRANSFORM as a point
// transform (generic.rs:105-115), clamp to [0,1], powf(2.2); alpha 1.
MRT_HD V4 ycbcr(V4 luma, V4 chroma) {
  constexpr float KR = 0.2126f, KG = 0.7152f, KB = 0.0722f;
  const M4 m{V4{1.0f, 1.0f, 1.0f, 0.0f}, V4{0.0f, -(KB / KG) * (2.0f - 2.0f * KB), 2.0f - 2.0f * KB, 0.0f},
             V4{2.0f - 2.0f * KR, -(KR / KG) * (2.0f - 2.0f * KR), 0.0f, 0.0f}, V4{0.0f, 0.0f, 0.0f, 1.0f}};
  V3 c = transform(m, V3{luma.x, chroma.x - 0.5f, chroma.y - 0.5f}, 1.0f);
  c = V3{fmaxf(fminf(c.x, 1.0f), 0.0f), fmaxf(fminf(c.y, 1.0f), 0.0f), fmaxf(fminf(c.z, 1.0f), 0.0f)};
  return V4{powf(c.x, 2.2f), powf(c.y, 2.2f), powf(c.z, 2.2f), 1.0f};
}
MRT_HD V4 vmin4(V4 a, V4 b) { return V4{fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w)}; }
MRT_HD V4 vmax4(V4 a, V4 b) { return V4{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)}; }

// A composite surface's postfix program (layout.h). The operand stack is
// kSurfStack registers shifted on push/pop (static indices only, so it never
// lives in scratch); only the EXT kernel variants contain this code.
MRT_HD V4 surface_program(const DevScene& S, uint32_t start, uint32_t len, V2 uv, LocalCounters& lc) {
  static_assert(kSurfStack == 4, "stack shifts below are written for 4 slots");
  V4 s0{}, s1{}, s2{}, s3{};
  for (uint32_t i = 0; i < len; ++i) {
    const GpuSurfOp o = S.surf_ops[MRT_IDX(S, start + i, S.n_surf_ops, 17)];
    const V4 color{o.color[0], o.color[1], o.color[2], o.color[3]};
    if (o.op == MRT_SURF_SOLID || o.op == MRT_SURF_TEXTURE) {  // push
      const V4 v = o.op == MRT_SURF_TEXTURE ? texture_get_f(S, o.tex, uv, lc) : color;
      s3 = s2, s2 = s1, s1 = s0, s0 = v;
    } else if (o.op == MRT_SURF_FALLBACK) {  // SolidColorFallback::get_f (texture.rs:353-356)
      s0 = (color * (1.0f - s0.w)) + (s0 * s0.w);
    } else {  // binary: left = s1, right = s0
      V4 v;
      if (o.op == MRT_SURF_YCBCR) v = ycbcr(s1, s0);
      else if (o.arg == MRT_BLEND_LIGHTEN) v = vmax4(s1, s0);  // BlendMode::blend (texture.rs:260-267)
      else if (o.arg == MRT_BLEND_DARKEN) v = vmin4(s1, s0);
      else if (o.arg == MRT_BLEND_ADDITION) v = vmin4(s1 + s0, V4{1.0f, 1.0f, 1.0f, 1.0f});
      else v = vmax4(s1 - s0, V4{0.0f, 0.0f, 0.0f, 0.0f});
      s0 = v, s1 = s2, s2 = s3;
    }
  }
  return s0;
}

template <bool EXT>
MRT_HD V4 surface_ref_get_f(const DevScene& S, uint32_t kind, uint32_t index, uint32_t len, const float* color,
                             V2 uv, LocalCounters& lc) {
  if (kind == MRT_SURF_TEXTURE) return texture_get_f(S, index, uv, lc);
  if (EXT && kind == SURF_PROGRAM) return surface_program(S, index, len, uv, lc);
  return V4{color[0], color[1], color[2], color[3]};
}

template <bool EXT>
MRT_HD V4 surface_get_f(const DevScene& S, const GpuMaterial& m, V2 uv, LocalCounters& lc) {
  return surface_ref_get_f<EXT>(S, m.surf_kind, m.texture, m.surf_len, m.color, uv, lc);
}

}  // namespace mrt
