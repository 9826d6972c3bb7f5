// denoise.hip — the Denoise display mode (main.rs:675-683, 724-747): a guided
// à-trous filter (Dammertz et al. 2010) where the reference calls Intel OIDN.
// OIDN is a neural filter and cannot be restated; this one keeps its call
// shape — noisy LDR colour plus the pre-pass albedo and normal in, filtered
// colour out, then the Default byte mapping — and is specified operation by
// operation (include/massrt.h, mrt_denoise_device), so the device result
// equals a host restatement bit for bit (tests/denoise_ref.py). With 0
// iterations it is the reference's own Denoise mode without the `denoise`
// feature: the Default view.
//
// The filter is for low sample counts. At the default widths it roughly
// halves the error of a 4-16 spp image and over-smooths from about 64 spp
// on; callers with more samples lower sigma_color.
//
// k_denoise_prep turns the sums into one float4 of prepared colour per pixel
// and one 32-B guide record {a.xyz, n.x}{n.yz, 0, 0}; an iteration is one
// pixel per thread, a wave being 64 consecutive x of one row, so each of a
// tap's three 16-B loads is 1 KiB contiguous per wave. Steps 1 and 2 read
// their taps from an LDS-staged tile (k_denoise_iter_lds), the later steps
// from global memory (k_denoise_iter); both run dn_filter, the one statement
// of the arithmetic.
#include <math.h>

#include <algorithm>

#include "ctx.h"
#include "display_math.h"

using namespace mrt;

namespace {

constexpr uint32_t kDnTileW = 64, kDnTileH = kBlock / 64;  // a workgroup's pixels: one wave per row
constexpr uint32_t kDnMaxIterations = 8;
constexpr uint32_t kDnColour = 1, kDnAlbedo = 2, kDnNormal = 4;  // the weight terms in effect

// The pixel of this thread in tile t (tiles in raster order); false outside the image.
__device__ __forceinline__ bool dn_pixel(uint64_t t, uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t& x,
                                         uint32_t& y) {
  const uint64_t ty = t / tiles_x, tx = t - ty * tiles_x;
  const uint64_t px = tx * kDnTileW + (threadIdx.x & 63u), py = ty * kDnTileH + (threadIdx.x >> 6);
  x = (uint32_t)px, y = (uint32_t)py;
  return px < W && py < H;
}

// c0 of a colour sum: gamma_byte's own domain rule (passes.hip), so the byte of c0 is Default's byte
__device__ __forceinline__ float dn_colour(float scale, float sum) {
  const float v = scale * sum;
  return (!(v >= 0.0f) || v > 1.0f) ? 1.0f : v;
}

template <bool AUX>
__global__ __launch_bounds__(kBlock) void k_denoise_prep(uint32_t W, uint32_t H, uint32_t tiles_x, uint64_t tiles,
                                                         const float* __restrict__ sum, float scale,
                                                         const float* __restrict__ albedo,
                                                         const float* __restrict__ normal,
                                                         float4* __restrict__ colour, float4* __restrict__ guides,
                                                         float* __restrict__ out3) {
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint32_t x, y;
    if (!dn_pixel(t, tiles_x, W, H, x, y)) continue;
    const size_t p = (size_t)y * W + x;
    const float r = dn_colour(scale, sum[3 * p]), g = dn_colour(scale, sum[3 * p + 1]),
                b = dn_colour(scale, sum[3 * p + 2]);
    if (out3) {  // 0 iterations: the prepared colour is the output
      out3[3 * p] = r, out3[3 * p + 1] = g, out3[3 * p + 2] = b;
      continue;
    }
    colour[p] = make_float4(r, g, b, 0.0f);
    if (AUX) {
      const float ar = rs_max(rs_min(albedo[3 * p], 1.0f), 0.0f), ag = rs_max(rs_min(albedo[3 * p + 1], 1.0f), 0.0f),
                  ab = rs_max(rs_min(albedo[3 * p + 2], 1.0f), 0.0f);
      guides[2 * p] = make_float4(ar, ag, ab, normal[3 * p]);
      guides[2 * p + 1] = make_float4(normal[3 * p + 1], normal[3 * p + 2], 0.0f, 0.0f);
    }
  }
}

__device__ __forceinline__ float dn_fall(float t) {
  const float u = 1.0f - t;
  return t < 1.0f ? u * u : 0.0f;  // NaN -> 0
}
__device__ __forceinline__ float dn_dist(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The reciprocal widths of one iteration and which weight terms are on.
struct DnWidths {
  float inv_c, inv_a, inv_n;
  uint32_t terms;
};

// One pixel of one à-trous iteration at step s: the 25 taps dy outer, dx
// inner; that order, and the order of every operation below, is the contract.
// tap(dx, dy, qx, qy, cq, gq0, gq1) fetches the in-image tap q = (qx, qy).
template <bool AUX, typename Tap>
__device__ __forceinline__ float4 dn_filter(uint32_t x, uint32_t y, uint32_t W, uint32_t H, uint32_t s,
                                            const DnWidths& wd, const float4 cp, const float4 gp0, const float4 gp1,
                                            Tap&& tap) {
  constexpr float h[3] = {0.375f, 0.25f, 0.0625f};
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, sw = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const float k = h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy];
      float w = k;
      float4 cq = cp;
      if (dx != 0 || dy != 0) {
        const int64_t qx = (int64_t)x + (int64_t)dx * s, qy = (int64_t)y + (int64_t)dy * s;
        if (qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H) continue;  // no clamping, no mirroring
        float4 gq0 = gp0, gq1 = gp1;
        tap(dx, dy, qx, qy, cq, gq0, gq1);
        if (wd.terms & kDnColour) w = w * dn_fall(dn_dist(cq.x, cq.y, cq.z, cp.x, cp.y, cp.z) * wd.inv_c);
        if (AUX) {
          if (wd.terms & kDnAlbedo) w = w * dn_fall(dn_dist(gq0.x, gq0.y, gq0.z, gp0.x, gp0.y, gp0.z) * wd.inv_a);
          if (wd.terms & kDnNormal) w = w * dn_fall(dn_dist(gq0.w, gq1.x, gq1.y, gp0.w, gp1.x, gp1.y) * wd.inv_n);
        }
      }
      ar = ar + w * cq.x;
      ag = ag + w * cq.y;
      ab = ab + w * cq.z;
      sw = sw + w;
    }
  }
  return make_float4(ar / sw, ag / sw, ab / sw, 0.0f);  // sw >= 9/64: the centre tap
}

// The last iteration writes the packed output, the others the ping-pong buffer.
__device__ __forceinline__ void dn_store(size_t p, const float4 c, float4* __restrict__ cout,
                                         float* __restrict__ out3) {
  if (out3)
    out3[3 * p] = c.x, out3[3 * p + 1] = c.y, out3[3 * p + 2] = c.z;
  else
    cout[p] = c;
}

// Steps 4 and up: every tap from global memory (L1/L2 at step 4, the Infinity Cache beyond).
template <bool AUX>
__global__ __launch_bounds__(kBlock) void k_denoise_iter(uint32_t W, uint32_t H, uint32_t tiles_x, uint64_t tiles,
                                                         uint32_t s, DnWidths wd, const float4* __restrict__ cin,
                                                         const float4* __restrict__ guides,
                                                         float4* __restrict__ cout, float* __restrict__ out3) {
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint32_t x, y;
    if (!dn_pixel(t, tiles_x, W, H, x, y)) continue;
    const size_t p = (size_t)y * W + x;
    const float4 c = dn_filter<AUX>(x, y, W, H, s, wd, cin[p], AUX ? guides[2 * p] : zero,
                                    AUX ? guides[2 * p + 1] : zero,
                                    [&](int, int, int64_t qx, int64_t qy, float4& cq, float4& gq0, float4& gq1) {
                                      const size_t q = (size_t)qy * W + (size_t)qx;
                                      cq = cin[q];
                                      if (AUX) gq0 = guides[2 * q], gq1 = guides[2 * q + 1];
                                    });
    dn_store(p, c, cout, out3);
  }
}

// Steps S = 1 and 2: the workgroup's 64x4 pixels and their halo of 2*S are
// staged in LDS once (26 KiB at S = 1, 41 KiB at S = 2 with guides), so a tap
// is three ds_read_b128 where k_denoise_iter issues three global loads. At
// these steps neighbouring pixels share most taps; measured at 1920x1080 with
// guides, preparation plus these two iterations take 0.20 ms this way against
// 0.30 ms (profiles/denoise_lds). From step 4 on the halo
// outgrows the tile.
template <bool AUX, int S>
__global__ __launch_bounds__(kBlock) void k_denoise_iter_lds(uint32_t W, uint32_t H, uint32_t tiles_x, uint64_t tiles,
                                                             DnWidths wd, const float4* __restrict__ cin,
                                                             const float4* __restrict__ guides,
                                                             float4* __restrict__ cout, float* __restrict__ out3) {
  constexpr int TW = (int)kDnTileW + 4 * S, TH = (int)kDnTileH + 4 * S;
  __shared__ float4 sc[TW * TH];
  __shared__ float4 sg0[AUX ? TW * TH : 1], sg1[AUX ? TW * TH : 1];
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const int64_t ox = (int64_t)(tx * kDnTileW) - 2 * S, oy = (int64_t)(ty * kDnTileH) - 2 * S;
    for (int i = (int)threadIdx.x; i < TW * TH; i += kBlock) {
      const int ly = i / TW, lx = i - ly * TW;
      const int64_t gx = ox + lx, gy = oy + ly;
      if (gx < 0 || gx >= (int64_t)W || gy < 0 || gy >= (int64_t)H) continue;  // never read: dn_filter skips the tap
      const size_t q = (size_t)gy * W + (size_t)gx;
      sc[i] = cin[q];
      if (AUX) sg0[i] = guides[2 * q], sg1[i] = guides[2 * q + 1];
    }
    __syncthreads();
    uint32_t x, y;
    if (dn_pixel(t, tiles_x, W, H, x, y)) {
      // this pixel in the stage; tap (dx, dy) lies dy*S rows and dx*S columns from it, inside the halo
      const int lc = ((int)(threadIdx.x >> 6) + 2 * S) * TW + (int)(threadIdx.x & 63u) + 2 * S;
      const float4 c = dn_filter<AUX>(x, y, W, H, (uint32_t)S, wd, sc[lc], AUX ? sg0[lc] : zero, AUX ? sg1[lc] : zero,
                                      [&](int dx, int dy, int64_t, int64_t, float4& cq, float4& gq0, float4& gq1) {
                                        const int lq = lc + dy * S * TW + dx * S;
                                        cq = sc[lq];
                                        if (AUX) gq0 = sg0[lq], gq1 = sg1[lq];
                                      });
      dn_store((size_t)y * W + x, c, cout, out3);
    }
    __syncthreads();  // the next tile overwrites the stage
  }
}

// 1 / sigma^2 in f32; sigma <= 0 switches the term off (`on` false)
float dn_inv(float sigma, bool& on) {
  on = sigma > 0.0f;
  return on ? 1.0f / (sigma * sigma) : 0.0f;
}

void denoise_check(uint32_t W, uint32_t H, const float* rgb, const float* albedo, const float* normal,
                   const mrt_denoise_params* params, const float* out) {
  check_image_size(W, H);
  if (!rgb || !out) throw ApiError{MRT_ERR_INVALID, "null buffer"};
  if ((albedo == nullptr) != (normal == nullptr))
    throw ApiError{MRT_ERR_INVALID, "albedo and normal go together: both or neither"};
  if (out == rgb || (albedo && (out == albedo || out == normal)))
    throw ApiError{MRT_ERR_INVALID, "the output buffer is one of the inputs"};
  if (params)
    if (const char* why = denoise_params_error(*params)) throw ApiError{MRT_ERR_INVALID, why};
}

}  // namespace

const char* denoise_params_error(const mrt_denoise_params& p) {
  if (p.iterations > kDnMaxIterations) return "denoise: at most 8 iterations";
  if (p.sigma_color != p.sigma_color || p.sigma_albedo != p.sigma_albedo || p.sigma_normal != p.sigma_normal)
    return "denoise: a sigma is NaN";
  return nullptr;
}

extern "C" {

int mrt_denoise_default_params(mrt_denoise_params* out) {
  if (!out) {
    mrt_global_error = "null output";
    return MRT_ERR_INVALID;
  }
  *out = mrt_denoise_params{5u, 2.0f, 0.3f, 0.6f};
  return MRT_OK;
}

int mrt_denoise_device(mrt_ctx* c, uint32_t W, uint32_t H, const float* d_rgb, uint32_t passes, const float* d_albedo,
                       const float* d_normal, const mrt_denoise_params* params, float* d_out, void* stream) {
  MRT_DEV0(c, mrt_denoise_device(c, W, H, d_rgb, passes, d_albedo, d_normal, params, d_out, stream));
  return guarded(c, [&] {
    denoise_check(W, H, d_rgb, d_albedo, d_normal, params, d_out);
    mrt_denoise_params prm;
    mrt_denoise_default_params(&prm);
    if (params) prm = *params;
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream (ordered with the caller's default-stream work)
    const size_t n = (size_t)W * H;
    if (passes == 0) {  // main.rs:647
      HIP_CHECK(hipMemsetAsync(d_out, 0, n * 12, st));
      return;
    }
    const uint32_t tiles_x = (W + kDnTileW - 1) / kDnTileW;
    const uint64_t tiles = (uint64_t)tiles_x * ((H + kDnTileH - 1) / kDnTileH);
    const dim3 grid((uint32_t)std::min<uint64_t>(tiles, 1u << 20)), block(kBlock);
    const float scale = 1.0f / (float)passes;
    if (prm.iterations == 0) {
      hipLaunchKernelGGL(k_denoise_prep<false>, grid, block, 0, st, W, H, tiles_x, tiles, d_rgb, scale,
                         (const float*)nullptr, (const float*)nullptr, (float4*)nullptr, (float4*)nullptr, d_out);
      HIP_CHECK(hipGetLastError());
      return;
    }
    HIP_CHECK(c->dn_mem.reserve(4 * n));  // grows on demand, reused across calls
    float4 *colA = c->dn_mem.p, *colB = colA + n, *guides = colB + n;
    const bool aux = d_albedo != nullptr;
    if (aux)
      hipLaunchKernelGGL(k_denoise_prep<true>, grid, block, 0, st, W, H, tiles_x, tiles, d_rgb, scale, d_albedo,
                         d_normal, colA, guides, (float*)nullptr);
    else
      hipLaunchKernelGGL(k_denoise_prep<false>, grid, block, 0, st, W, H, tiles_x, tiles, d_rgb, scale,
                         (const float*)nullptr, (const float*)nullptr, colA, (float4*)nullptr, (float*)nullptr);
    HIP_CHECK(hipGetLastError());
    bool on_a, on_n;
    const float inv_a = dn_inv(prm.sigma_albedo, on_a), inv_n = dn_inv(prm.sigma_normal, on_n);
    for (uint32_t i = 0; i < prm.iterations; ++i) {
      bool on_c;
      const float inv_c = dn_inv(prm.sigma_color * ldexpf(1.0f, -(int)i), on_c);  // the colour width halves per iteration
      const DnWidths wd{inv_c, inv_a, inv_n,
                        (on_c ? kDnColour : 0u) | (on_a ? kDnAlbedo : 0u) | (on_n ? kDnNormal : 0u)};
      const float4* in = (i & 1u) ? colB : colA;
      float4* out = (i & 1u) ? colA : colB;
      float* out3 = i + 1 == prm.iterations ? d_out : nullptr;
      if (i < 2) {  // steps 1 and 2: taps from an LDS-staged tile
        auto* k = aux ? (i ? k_denoise_iter_lds<true, 2> : k_denoise_iter_lds<true, 1>)
                      : (i ? k_denoise_iter_lds<false, 2> : k_denoise_iter_lds<false, 1>);
        hipLaunchKernelGGL(k, grid, block, 0, st, W, H, tiles_x, tiles, wd, in, (const float4*)guides, out, out3);
      } else {
        hipLaunchKernelGGL(aux ? k_denoise_iter<true> : k_denoise_iter<false>, grid, block, 0, st, W, H, tiles_x,
                           tiles, 1u << i, wd, in, (const float4*)guides, out, out3);
      }
      HIP_CHECK(hipGetLastError());
    }
  });
}

int mrt_denoise(mrt_ctx* c, uint32_t W, uint32_t H, const float* rgb, uint32_t passes, const float* albedo,
                const float* normal, const mrt_denoise_params* params, float* out) {
  MRT_DEV0(c, mrt_denoise(c, W, H, rgb, passes, albedo, normal, params, out));
  return guarded(c, [&] {
    denoise_check(W, H, rgb, albedo, normal, params, out);
    const size_t n = (size_t)W * H;
    DevBuf<float> d;
    HIP_CHECK(d.alloc(n * 3 * (albedo ? 4 : 2)));
    float *d_rgb = d.p, *d_out = d.p + 3 * n, *d_albedo = albedo ? d.p + 6 * n : nullptr,
          *d_normal = albedo ? d.p + 9 * n : nullptr;
    HIP_CHECK(hipMemcpyAsync(d_rgb, rgb, n * 12, hipMemcpyHostToDevice, c->stream));
    if (albedo) {
      HIP_CHECK(hipMemcpyAsync(d_albedo, albedo, n * 12, hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(hipMemcpyAsync(d_normal, normal, n * 12, hipMemcpyHostToDevice, c->stream));
    }
    const int rc = mrt_denoise_device(c, W, H, d_rgb, passes, d_albedo, d_normal, params, d_out, c->stream);
    if (rc != MRT_OK) throw ApiError{rc, c->err};
    HIP_CHECK(hipMemcpyAsync(out, d_out, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
  });
}

}  // extern "C"
