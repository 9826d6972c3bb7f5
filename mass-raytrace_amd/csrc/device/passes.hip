// passes.hip — the passes around the integrator: tonemap, the albedo/normal pre-pass,
// the tile-slab exchange of sharded images, the arithmetic selftests; their entry points.
#include <algorithm>

#include "../host/display.h"
#include "ctx.h"
#include "display_math.h"

using namespace mrt;

namespace {

// div_cr (isect.h) against the IEEE division on random bit patterns plus
// structured operands (all-ones / power-of-two mantissas, range edges).
__global__ __launch_bounds__(kBlock) void k_selftest_division(unsigned long long n, unsigned long long seed,
                                                              unsigned long long* mismatches) {
  unsigned long long bad = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
  for (unsigned long long i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint64_t x = seed ^ (i * 0x9E3779B97F4A7C15ull);
    unsigned long long r1 = splitmix64_next(x), r2 = splitmix64_next(x);
    uint32_t ua = (uint32_t)r1, ub = (uint32_t)(r1 >> 32);
    switch (r2 & 7) {
      case 0:  // all-ones divisor mantissa
        ub |= 0x007FFFFFu;
        break;
      case 1:  // power-of-two divisor
        ub &= 0xFF800000u;
        break;
      case 2:  // all-ones dividend mantissa
        ua |= 0x007FFFFFu;
        break;
      case 3:  // scene-like magnitudes: exponents near 1
        ua = (ua & 0x807FFFFFu) | ((120u + ((uint32_t)(r2 >> 8) % 20u)) << 23);
        ub = (ub & 0x807FFFFFu) | ((110u + ((uint32_t)(r2 >> 16) % 30u)) << 23);
        break;
      case 4:  // quotient near 1 ulp ties: a = b * small integer
        ub = (ub & 0x807FFFFFu) | (127u << 23);
        {
          float fa = __uint_as_float(ub) * (float)((r2 >> 8) & 0xFFFF);
          ua = __float_as_uint(fa) ^ (uint32_t)((r2 >> 32) & 3);
        }
        break;
      default:
        break;
    }
    float a = __uint_as_float(ua), b = __uint_as_float(ub);
    float q;
    if ((r2 & 7) >= 5) {
      // the slab test's fast domain (isect.h TRay): a = m - o with m, o in
      // {0} U [2^-40, 2^28], |b| in [2^-20, 2^20]; q = qfast(a, b, RN(1/b))
      auto coord = [](uint32_t bits, uint32_t sel) {
        uint32_t e = 87u + (sel % 68u);  // 2^-40 .. 2^27
        float v = __uint_as_float((bits & 0x807FFFFFu) | (e << 23));
        return (sel & 15u) == 0 ? 0.0f : v;
      };
      float m = coord(ua, (uint32_t)(r2 >> 8)), o = coord(ub, (uint32_t)(r2 >> 24));
      if ((r2 >> 40) & 1) o = m;  // zero numerators
      if (((r2 >> 42) & 3) == 0 && m != 0.0f)  // cancellation: o a few ulps from m
        o = __uint_as_float(__float_as_uint(m) + (uint32_t)((r2 >> 44) & 7));
      a = m - o;
      uint32_t eb = 107u + ((uint32_t)(r2 >> 48) % 40u);  // 2^-20 .. 2^19
      b = __uint_as_float((ub & 0x807FFFFFu) | (eb << 23));
      q = qfast(a, b, 1.0f / b);
    } else {
      q = div_cr(a, make_recip(b));
    }
    float ref = a / b;
    uint32_t uq = __float_as_uint(q), ur = __float_as_uint(ref);
    bool same = uq == ur || (q != q && ref != ref) || (q == 0.0f && ref == 0.0f);
    bad += same ? 0 : 1;
  }
  bad = (unsigned long long)wave_sum((uint32_t)bad);
  if (lane_id() == 0 && bad) atomicAdd(mismatches, bad);
}

// ---- display (main.rs:640-722, 760-767) ----------------------------------
// Rust f32::min/max and saturating `as u8`: display_math.h.
// Default-mode byte of x = sum/passes: the count of thresholds <= x for x in
// [0, 1] (-0.0 counts as 0); NaN or negative x -> NaN.powf -> .min(1.0) = 1.0
// -> 255; -inf.powf = +inf and x > 1 -> 255.
// t: host/display.h's table, t[k] = bits of the smallest x in [0,1] whose byte is >= k
__device__ __forceinline__ uint32_t gamma_byte(const uint32_t* t, float x) {
  if (!(x >= 0.0f) || x > 1.0f) return 255u;
  const uint32_t u = __float_as_uint(x) & 0x7FFFFFFFu;  // -0.0 -> powf gives +0 -> byte 0
  uint32_t lo = 0;  // largest k with t[k] <= u (t[0] = 0 <= u)
#pragma unroll
  for (uint32_t step = 128; step > 0; step >>= 1)
    if (t[lo + step] <= u) lo += step;  // lo + step <= 255
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_max_u32(const uint32_t* v, uint32_t n, uint32_t* out) {
  uint32_t m = 0;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) m = v[i] > m ? v[i] : m;
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if (lane_id() == 0) atomicMax(out, m);
}

// Tile-slab exchange (mrt_shard_*): slab k = the shard's k-th pixel.
__global__ __launch_bounds__(kBlock) void k_shard_pack(const uint32_t* pixlist, uint32_t n, const float* rgb,
                                                       const uint32_t* b, uint4* slab) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const uint32_t p = pixlist[k];
  slab[k] = make_uint4(__float_as_uint(rgb[3 * (size_t)p]), __float_as_uint(rgb[3 * (size_t)p + 1]),
                       __float_as_uint(rgb[3 * (size_t)p + 2]), b[p]);
}
__global__ __launch_bounds__(kBlock) void k_shard_unpack(const uint32_t* pixlist, uint32_t n, const uint4* slab,
                                                         float* rgb, uint32_t* b) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const uint32_t p = pixlist[k];
  const uint4 v = slab[k];
  rgb[3 * (size_t)p] = __uint_as_float(v.x);
  rgb[3 * (size_t)p + 1] = __uint_as_float(v.y);
  rgb[3 * (size_t)p + 2] = __uint_as_float(v.z);
  b[p] = v.w;
}

// Camera::albedo_normal for pixel p (one ray, no jitter). The rays go through
// ray_ro/ray_rd so that the traversal can re-read them (TravIn).
template <bool RNG, bool EXT>
__global__ __launch_bounds__(kBlock) void k_prepass(DevScene S, DevCamera cam, uint32_t W, uint32_t H,
                                                    unsigned long long seed, float4* ray_ro, float4* ray_rd,
                                                    float* albedo, float* normal) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= W * H) return;
  const uint32_t y = p / W, x = p - y * W;
  PathRng rng = path_rng(seed, p, 0xFFFFFFFFu);
  V3 o, d;
  camera_ray_uv(cam, (float)x / (float)(W - 1), (float)y / (float)(H - 1), rng, o, d);
  ray_ro[p] = make_float4(o.x, o.y, o.z, 0.0f);
  ray_rd[p] = make_float4(d.x, d.y, d.z, 0.0f);
  const TravIn tin{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, ray_ro, ray_rd, kTmin};
  LocalCounters lc;
  const Hit h = closest_hit<false, RNG, EXT>(tin, p, INFINITY, lc, rng);
  V3 a{0.0f, 0.0f, 0.0f}, n{0.0f, 0.0f, 0.0f};
  if (h.prim != kRefNone) {
    Surf s = resolve_hit<EXT>(S, o, d, h, lc);
    V3 emitted, atten, nd;
    uint32_t mkind;
    a = scatter<EXT>(S, s, d, rng, emitted, atten, nd, lc, mkind) ? atten : emitted;
    n = s.normal;
  } else {
    a = background<EXT>(S, d, lc);
  }
  albedo[3 * (size_t)p] = a.x, albedo[3 * (size_t)p + 1] = a.y, albedo[3 * (size_t)p + 2] = a.z;
  normal[3 * (size_t)p] = n.x, normal[3 * (size_t)p + 1] = n.y, normal[3 * (size_t)p + 2] = n.z;
}

// mrt_shade_rays: ray i traced and shaded one step (a test entry point, not
// hot). One stream per ray: the traversal's draws, emit's, scatter's.
template <bool RNG, bool EXT>
__global__ __launch_bounds__(kBlock) void k_shade_rays(DevScene S, const float* rays, uint32_t n, float tmin,
                                                       float tmax, unsigned long long seed, float4* ray_ro,
                                                       float4* ray_rd, mrt_shade_out* out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * (size_t)i;
  const V3 o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
  ray_ro[i] = make_float4(o.x, o.y, o.z, 0.0f);
  ray_rd[i] = make_float4(d.x, d.y, d.z, 0.0f);
  PathRng rng = path_rng(seed, i, 0xFFFFFFFDu);
  const TravIn tin{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, ray_ro, ray_rd, tmin};
  LocalCounters lc;
  const Hit h = closest_hit<false, RNG, EXT>(tin, i, tmax, lc, rng);
  mrt_shade_out w{};
  if (h.prim != kRefNone) {
    const Surf s = resolve_hit<EXT>(S, o, d, h, lc);
    V3 emitted, atten{0, 0, 0}, nd{0, 0, 0};
    uint32_t mkind;
    const bool cont = scatter<EXT>(S, s, d, rng, emitted, atten, nd, lc, mkind);
    w.prim = h.prim, w.container = h.container, w.t = h.t;
    w.flags = (s.front_face ? MRT_SHADE_FRONT_FACE : 0u) | (s.has_uv ? MRT_SHADE_HAS_UV : 0u) |
              (cont ? MRT_SHADE_SCATTERED : 0u);
    w.point[0] = s.point.x, w.point[1] = s.point.y, w.point[2] = s.point.z;
    w.normal[0] = s.normal.x, w.normal[1] = s.normal.y, w.normal[2] = s.normal.z;
    w.uv[0] = s.has_uv ? s.uv.x : 0.0f, w.uv[1] = s.has_uv ? s.uv.y : 0.0f;
    w.material = s.material;
    w.emitted[0] = emitted.x, w.emitted[1] = emitted.y, w.emitted[2] = emitted.z;
    if (cont) {
      w.attenuation[0] = atten.x, w.attenuation[1] = atten.y, w.attenuation[2] = atten.z;
      w.direction[0] = nd.x, w.direction[1] = nd.y, w.direction[2] = nd.z;
    }
  }
  out[i] = w;
}

// One thread per pixel; writes the pixel's 3 bytes at the flipped row.
__global__ __launch_bounds__(kBlock) void k_tonemap(uint32_t W, uint32_t H, const float* rgb, const uint32_t* b,
                                                    uint32_t passes, uint32_t mode, const uint32_t* max_count,
                                                    const uint32_t* g, uint8_t* out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= W * H) return;
  const uint32_t y = p / W, x = p - y * W;
  uint8_t* dst = out + ((size_t)(H - 1 - y) * W + x) * 3;
  if (mode == MRT_DISPLAY_ALBEDO || mode == MRT_DISPLAY_NORMAL) {  // main.rs:689-718
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = rgb[3 * (size_t)p + c];
      if (mode == MRT_DISPLAY_NORMAL) {
        dst[c] = (uint8_t)rs_u8(((v + 1.0f) / 2.0f) * 255.0f);
      } else {  // p.min(1).max(0).powf(1/2.2): NaN -> 1 -> 255, <= 0 -> 0
        const float q = rs_max(rs_min(v, 1.0f), 0.0f);
        dst[c] = (uint8_t)(q >= 1.0f ? 255u : gamma_byte(g, q));
      }
    }
    return;
  }
  if (passes == 0) {
    dst[0] = dst[1] = dst[2] = 0;
    return;
  }
  const float scale = 1.0f / (float)passes;
  if (mode == MRT_DISPLAY_DEPTH) {
    const uint32_t m = *max_count;
    const float max_depth = (float)(m > 1u ? m : 1u) * scale;
    const float d = rs_min(rs_max(((float)b[p] * scale) / max_depth, 0.0f), 1.0f);
    dst[0] = dst[1] = dst[2] = (uint8_t)rs_u8(d * 255.0f);
  } else {
    dst[0] = (uint8_t)gamma_byte(g, scale * rgb[3 * (size_t)p]);
    dst[1] = (uint8_t)gamma_byte(g, scale * rgb[3 * (size_t)p + 1]);
    dst[2] = (uint8_t)gamma_byte(g, scale * rgb[3 * (size_t)p + 2]);
  }
}

// box_hit_any (early decision + exact fallback) against box_hit_exact on
// rays in the fast domain and boxes whose faces pass within a few ulps of a
// point of the ray (entry/exit ties), flat boxes, and t_max near the faces.
__global__ __launch_bounds__(kBlock) void k_selftest_slab(unsigned long long n, unsigned long long seed,
                                                          unsigned long long* out) {
  unsigned long long bad = 0, ties = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
  for (unsigned long long i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint64_t x = seed ^ (i * 0xD1B54A32D192ED03ull);
    auto rnd = [&]() { return splitmix64_next(x); };
    auto coord = [&](uint64_t r) {  // {0} U [2^-40, 2^27], random sign
      uint32_t e = 87u + (uint32_t)((r >> 32) % 68u);
      float v = __uint_as_float(((uint32_t)r & 0x807FFFFFu) | (e << 23));
      return ((r >> 60) & 15u) == 0 ? 0.0f : v;
    };
    auto dir = [&](uint64_t r) {  // |d| in [2^-20, 2^19]
      uint32_t e = 107u + (uint32_t)((r >> 32) % 40u);
      return __uint_as_float(((uint32_t)r & 0x807FFFFFu) | (e << 23));
    };
    auto nudge = [](float v, int k) { return __uint_as_float(__float_as_uint(v) + k); };
    V3 o{coord(rnd()), coord(rnd()), coord(rnd())};
    const uint64_t sc = rnd();
    if (sc & 1) {  // scene-like magnitudes
      o = V3{(float)((int)(sc >> 8 & 255) - 128) * 0.37f, (float)((int)(sc >> 16 & 255) - 128) * 0.11f,
             (float)((int)(sc >> 24 & 255) - 128) * 0.23f};
    }
    V3 d{dir(rnd()), dir(rnd()), dir(rnd())};
    const float t = __uint_as_float((uint32_t)(((uint64_t)100u + (rnd() % 37u)) << 23) | ((uint32_t)rnd() & 0x7FFFFFu));
    const V3 p = o + d * t;
    float mn[3], mx[3];
    const float pv[3] = {p.x, p.y, p.z};
    for (int k = 0; k < 3; ++k) {
      const uint64_t r = rnd();
      const int a = (int)(r & 7), b = (int)((r >> 3) & 7);
      const float lo = (r >> 6 & 3) == 0 ? pv[k] - fabsf(pv[k]) * 0.25f - 0.5f : nudge(pv[k], -a);
      const float hi = (r >> 8 & 3) == 0 ? pv[k] + fabsf(pv[k]) * 0.25f + 0.5f : nudge(pv[k], b);
      mn[k] = fminf(lo, hi);
      mx[k] = fmaxf(lo, hi);
      if ((r >> 10 & 7) == 0) mx[k] = mn[k];  // flat box
    }
    // every 8th case: some box minima replaced by a tiny nonzero coordinate
    // (~1e-16, a mesh vertex at sin(pi)): outside the qfast domain, inside the
    // early decision's; the exact test then divides
    if ((sc >> 40 & 7) == 0)
      for (int k = 0; k < 3; ++k)
        if (rnd() & 1) mn[k] = fminf(mx[k], __uint_as_float((__float_as_uint(mn[k]) & 0x80000000u) | 0x25100000u));
    bool ok = true, early = true;
    for (int k = 0; k < 3; ++k) ok = ok && coord_ok(mn[k]) && coord_ok(mx[k]);
    for (int k = 0; k < 3; ++k) early = early && orig_ok(mn[k]) && orig_ok(mx[k]);
    if (!early) continue;
    const TRay ray = make_tray(o, d, ok ? 3u : 2u);
    if (!tray_fast(ray)) continue;
    const uint64_t rt = rnd();
    const float tmin = (rt & 3) == 0 ? nudge(t, -(int)(rt >> 2 & 3)) : 0.001f;
    const float tmax = (rt >> 4 & 3) == 0 ? INFINITY : ((rt >> 4 & 3) == 1 ? nudge(t, (int)(rt >> 6 & 7) - 3) : t * 2.0f);
    const V3 bmn{mn[0], mn[1], mn[2]}, bmx{mx[0], mx[1], mx[2]};
    const bool e = box_hit_exact(bmn, bmx, ray, tmin, tmax);
    const bool f = box_hit_any(bmn, bmx, ray, tmin, tmax);
    bad += e != f;
    // count how often the exact fallback had to decide
    float t0, t1;
    slab_fast(bmn, bmx, ray, tmin, tmax, t0, t1);
    const float m = slab_margin(ray, t0, t1);
    ties += !(t1 - t0 > m) && !(t0 - t1 > m);
  }
  bad = (unsigned long long)wave_sum((uint32_t)bad);
  ties = (unsigned long long)wave_sum((uint32_t)ties);
  if (lane_id() == 0 && (bad || ties)) {
    atomicAdd(out, bad);
    atomicAdd(out + 1, ties);
  }
}

int shard_exchange(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc, const void* src_rgb,
                   const void* src_b, const void* slab, float* dst_rgb, uint32_t* dst_b, void* stream, bool pack) {
  return guarded(c, [&] {
    check_image_size(W, H);
    if (sc == 0) sc = 1;
    if (si >= sc) throw ApiError{MRT_ERR_INVALID, "shard_index >= shard_count"};
    if (!slab || (pack && (!src_rgb || !src_b)) || (!pack && (!dst_rgb || !dst_b)))
      throw ApiError{MRT_ERR_INVALID, "null buffer"};
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream (ordered with the caller's default-stream work)
    auto pl = pixlist(c, W, H, si, sc);
    if (pl.second == 0) return;
    const dim3 grid((pl.second + kBlock - 1) / kBlock);
    if (pack)
      hipLaunchKernelGGL(k_shard_pack, grid, dim3(kBlock), 0, st, pl.first, pl.second, (const float*)src_rgb,
                         (const uint32_t*)src_b, (uint4*)slab);
    else
      hipLaunchKernelGGL(k_shard_unpack, grid, dim3(kBlock), 0, st, pl.first, pl.second, (const uint4*)slab, dst_rgb,
                         dst_b);
    HIP_CHECK(hipGetLastError());
  });
}

// A selftest kernel's N counters: zeroed, the kernel run over (n, seed), read back.
template <size_t N, typename K>
void run_selftest(mrt_ctx* c, K kernel, uint64_t n, uint64_t seed, unsigned long long (&h)[N]) {
  DevBuf<unsigned long long> d;
  HIP_CHECK(d.alloc(N));
  HIP_CHECK(hipMemsetAsync(d.p, 0, N * 8, c->stream));
  hipLaunchKernelGGL(kernel, dim3(4096), dim3(kBlock), 0, c->stream, (unsigned long long)n, (unsigned long long)seed,
                     d.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h, d.p, N * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
}

}  // namespace

extern "C" {

int mrt_selftest_division(mrt_ctx* c, uint64_t n, uint64_t seed, uint64_t* mismatches) {
  MRT_DEV0(c, mrt_selftest_division(c, n, seed, mismatches));
  return guarded(c, [&] {
    if (!mismatches) throw ApiError{MRT_ERR_INVALID, "null output"};
    unsigned long long h[1];
    run_selftest(c, k_selftest_division, n, seed, h);
    *mismatches = h[0];
  });
}

int mrt_tonemap_device(mrt_ctx* c, uint32_t W, uint32_t H, const float* d_rgb, const uint32_t* d_b, uint32_t passes,
                       uint32_t mode, uint8_t* d_out, void* stream) {
  MRT_DEV0(c, mrt_tonemap_device(c, W, H, d_rgb, d_b, passes, mode, d_out, stream));
  return guarded(c, [&] {
    check_image_size(W, H);
    if (mode > MRT_DISPLAY_NORMAL) throw ApiError{MRT_ERR_INVALID, "bad display mode"};
    const bool aux = mode == MRT_DISPLAY_ALBEDO || mode == MRT_DISPLAY_NORMAL;
    if (!d_out || (aux && !d_rgb) ||
        (passes && ((mode == MRT_DISPLAY_DEFAULT && !d_rgb) || (mode == MRT_DISPLAY_DEPTH && !d_b))))
      throw ApiError{MRT_ERR_INVALID, "null buffer"};
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream (ordered with the caller's default-stream work)
    const uint32_t n = W * H;
    if (!c->gamma_d.p) {
      HIP_CHECK(c->gamma_d.alloc(256));
      HIP_CHECK(hipMemcpy(c->gamma_d.p, mrt::gamma_thresholds().data(), 256 * 4, hipMemcpyHostToDevice));
    }
    uint32_t* d_max = c->work.p + 1;  // word 1 of the work line: max count
    HIP_CHECK(hipMemsetAsync(d_max, 0, 4, st));
    if (mode == MRT_DISPLAY_DEPTH && passes) {
      hipLaunchKernelGGL(k_max_u32, dim3(std::min<uint32_t>((n + kBlock - 1) / kBlock, 4096u)), dim3(kBlock), 0, st,
                         d_b, n, d_max);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tonemap, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, W, H, d_rgb, d_b, passes,
                       mode, (const uint32_t*)d_max, (const uint32_t*)c->gamma_d.p, d_out);
    HIP_CHECK(hipGetLastError());
  });
}

int mrt_tonemap(mrt_ctx* c, uint32_t W, uint32_t H, const float* rgb, const uint32_t* b, uint32_t passes,
                uint32_t mode, uint8_t* out) {
  MRT_DEV0(c, mrt_tonemap(c, W, H, rgb, b, passes, mode, out));
  return guarded(c, [&] {
    check_image_size(W, H);
    if (!out || !rgb || !b) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const size_t n = (size_t)W * H;
    DevBuf<char> mem;
    HIP_CHECK(mem.alloc(n * 12 + n * 4 + n * 3 + 256));
    float* d_rgb = (float*)mem.p;
    uint32_t* d_b = (uint32_t*)(d_rgb + 3 * n);
    uint8_t* d_out = (uint8_t*)(d_b + n);
    HIP_CHECK(hipMemcpyAsync(d_rgb, rgb, n * 12, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(d_b, b, n * 4, hipMemcpyHostToDevice, c->stream));
    const int rc = mrt_tonemap_device(c, W, H, d_rgb, d_b, passes, mode, d_out, c->stream);
    if (rc != MRT_OK) throw ApiError{rc, c->err};
    HIP_CHECK(hipMemcpyAsync(out, d_out, n * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
  });
}

int mrt_prepass_device(mrt_ctx* c, uint32_t W, uint32_t H, uint64_t seed, float* d_albedo, float* d_normal,
                       void* stream) {
  MRT_DEV0(c, mrt_prepass_device(c, W, H, seed, d_albedo, d_normal, stream));
  return guarded(c, [&] {
    if (!c->has_scene) throw ApiError{MRT_ERR_STATE, "no scene uploaded"};
    if (!c->has_camera) throw ApiError{MRT_ERR_STATE, "no camera set"};
    check_image_size(W, H);
    if (!d_albedo || !d_normal) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream (ordered with the caller's default-stream work)
    wait_queues(c, st);
    const uint32_t n = W * H;
    ensure_slots(c, n);  // the pre-pass rays
    auto* prepass = with_value<true, false>(c->facts.trav_rng, [&](auto RNG) {
      return with_value<true, false>(c->scene_ext, [&](auto EXT) { return &k_prepass<RNG, EXT>; });
    });
    hipLaunchKernelGGL(prepass, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, c->S, c->cam, W, H,
                       (unsigned long long)seed, c->slot_ro, c->slot_rd, d_albedo, d_normal);
    HIP_CHECK(hipGetLastError());
    mark_ctx_busy(c, st);  // the pre-pass rays live in slot_ro/slot_rd, which the drain hand-off reuses
  });
}

int mrt_prepass(mrt_ctx* c, uint32_t W, uint32_t H, uint64_t seed, float* albedo, float* normal) {
  MRT_DEV0(c, mrt_prepass(c, W, H, seed, albedo, normal));
  return guarded(c, [&] {
    check_image_size(W, H);
    if (!albedo || !normal) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const size_t n = (size_t)W * H;
    DevBuf<float> d;
    HIP_CHECK(d.alloc(n * 6));
    const int rc = mrt_prepass_device(c, W, H, seed, d.p, d.p + 3 * n, c->stream);
    if (rc != MRT_OK) throw ApiError{rc, c->err};
    HIP_CHECK(hipMemcpyAsync(albedo, d.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(normal, d.p + 3 * n, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
  });
}

int mrt_shade_rays(mrt_ctx* c, const float* rays, uint32_t n, float t_min, float t_max, uint64_t seed,
                   mrt_shade_out* out) {
  MRT_DEV0(c, mrt_shade_rays(c, rays, n, t_min, t_max, seed, out));
  return guarded(c, [&] {
    if (!c->has_scene) throw ApiError{MRT_ERR_STATE, "no scene uploaded"};
    if (n == 0) return;
    if (!rays || !out) throw ApiError{MRT_ERR_INVALID, "null argument"};
    wait_queues(c, c->stream);
    ensure_slots(c, n);  // the rays where the traversal re-reads them
    DevBuf<char> mem;
    const size_t ray_bytes = ((size_t)n * 24 + 255) & ~(size_t)255;
    HIP_CHECK(mem.alloc(ray_bytes + (size_t)n * sizeof(mrt_shade_out)));
    float* d_rays = (float*)mem.p;
    mrt_shade_out* d_out = (mrt_shade_out*)(mem.p + ray_bytes);
    HIP_CHECK(hipMemcpyAsync(d_rays, rays, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    auto* f = with_value<true, false>(c->facts.trav_rng, [&](auto RNG) {
      return with_value<true, false>(c->scene_ext, [&](auto EXT) { return &k_shade_rays<RNG, EXT>; });
    });
    hipLaunchKernelGGL(f, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S, (const float*)d_rays, n,
                       t_min, t_max, (unsigned long long)seed, c->slot_ro, c->slot_rd, d_out);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(mrt_shade_out), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    mark_ctx_busy(c, c->stream);  // slot_ro/slot_rd are shared with the drain hand-off
  });
}

int mrt_selftest_slab(mrt_ctx* c, uint64_t n, uint64_t seed, uint64_t* mismatches, uint64_t* near_ties) {
  MRT_DEV0(c, mrt_selftest_slab(c, n, seed, mismatches, near_ties));
  return guarded(c, [&] {
    if (!mismatches || !near_ties) throw ApiError{MRT_ERR_INVALID, "null output"};
    unsigned long long h[2];
    run_selftest(c, k_selftest_slab, n, seed, h);
    *mismatches = h[0];
    *near_ties = h[1];
  });
}

int mrt_shard_pack_device(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc, const float* d_rgb,
                          const uint32_t* d_b, void* d_slab, void* stream) {
  MRT_DEV0(c, mrt_shard_pack_device(c, W, H, si, sc, d_rgb, d_b, d_slab, stream));
  return shard_exchange(c, W, H, si, sc, d_rgb, d_b, d_slab, nullptr, nullptr, stream, true);
}

int mrt_shard_unpack_device(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc, const void* d_slab,
                            float* d_rgb, uint32_t* d_b, void* stream) {
  MRT_DEV0(c, mrt_shard_unpack_device(c, W, H, si, sc, d_slab, d_rgb, d_b, stream));
  return shard_exchange(c, W, H, si, sc, nullptr, nullptr, d_slab, d_rgb, d_b, stream, false);
}

}  // extern "C"
