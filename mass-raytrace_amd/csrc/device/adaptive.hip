// adaptive.hip — the kernels of mrt_render_adaptive for gfx950 (the rule is in
// include/massrt.h, its arithmetic in host/adaptive.h; the rounds around the
// wavefront loop are render.hip's render_adaptive_device):
//   k_accumulate_moments : k_accumulate that also adds y, y y and the count [per round]
//   k_adaptive_tiles     : the decision, one wave per tile                  [per round]
//   k_adaptive_scan_tiles, k_adaptive_scan_blocks, k_adaptive_compact :
//                          the open tiles' pixels in shard order -> the next
//                          round's pixel list and its length               [per round]
//   k_adaptive_resolve   : sums / per-pixel count
// and the entry points that need nothing of the wavefront loop.
#include <string.h>

#include <algorithm>

#include "../host/adaptive.h"
#include "ctx.h"
#include "devbase.h"

using namespace mrt;

namespace {

// MRT_IDX's record for a kernel that has no other struct to carry it (DevScene::dbg)
struct DbgRec {
  uint32_t* dbg;
};

// ---- accumulate with moments -------------------------------------------------

// k_accumulate's staging (render.hip): a workgroup sums kMomPix list pixels,
// blocks of kMomS samples of all of them go through LDS with coalesced loads
// (a pixel's samples are contiguous in the pixel-major slab), then each of the
// first kMomPix threads adds its pixel's samples in sample order: the colour
// and bounce sums take the very additions k_accumulate makes, and beside them
// y = (r + g) + b goes into m1, y y into m2 and one into the count.
constexpr uint32_t kMomPix = 64, kMomS = 16, kMomPad = kMomS + 1;  // +1 quad per row: no bank-aligned rows
struct MomOut {
  float* rgb;
  uint32_t* bounces;
  float* moments;
  uint32_t* samples;
  uint32_t n_frame;  // pixels of the frame: the bound of a list entry
  uint32_t* dbg;
};
__global__ __launch_bounds__(kBlock) void k_accumulate_moments(const float4* results, uint32_t n_pix,
                                                               uint32_t n_samples, const uint32_t* pixlist,
                                                               MomOut out) {
  __shared__ float4 tile[kMomPix * kMomPad];
  const uint32_t lp0 = blockIdx.x * kMomPix;
  const uint32_t n_here = n_pix - lp0 < kMomPix ? n_pix - lp0 : kMomPix;
  const uint32_t j = threadIdx.x;  // the pixel this thread sums (j < n_here)
  float r = 0.0f, g = 0.0f, b = 0.0f, m1 = 0.0f, m2 = 0.0f;
  uint32_t k = 0, n = 0, p = 0;
  if (j < n_here) {
    p = MRT_IDX(out, pixlist[MRT_IDX(out, lp0 + j, n_pix, 30)], out.n_frame, 31);
    r = out.rgb[3 * (size_t)p], g = out.rgb[3 * (size_t)p + 1], b = out.rgb[3 * (size_t)p + 2];
    k = out.bounces[p];
    m1 = out.moments[2 * (size_t)p], m2 = out.moments[2 * (size_t)p + 1];
    n = out.samples[p];
  }
  for (uint32_t s0 = 0; s0 < n_samples; s0 += kMomS) {
    const uint32_t sb = n_samples - s0 < kMomS ? n_samples - s0 : kMomS;
    for (uint32_t e = threadIdx.x; e < kMomPix * kMomS; e += kBlock) {
      const uint32_t px = e / kMomS, sx = e % kMomS;
      if (px < n_here && sx < sb)
        tile[px * kMomPad + sx] = results[MRT_IDX(out, (lp0 + px) * n_samples + s0 + sx, n_pix * n_samples, 32)];
    }
    __syncthreads();
    if (j < n_here) {
      for (uint32_t sx = 0; sx < sb; ++sx) {
        const float4 q = tile[j * kMomPad + sx];
        r = r + q.x;
        g = g + q.y;
        b = b + q.z;
        k += __float_as_uint(q.w);
        const float y = adapt_luma(q.x, q.y, q.z);
        m1 = m1 + y;
        m2 = m2 + y * y;
      }
    }
    __syncthreads();
  }
  if (j < n_here) {
    out.rgb[3 * (size_t)p] = r;
    out.rgb[3 * (size_t)p + 1] = g;
    out.rgb[3 * (size_t)p + 2] = b;
    out.bounces[p] = k;
    out.moments[2 * (size_t)p] = m1;
    out.moments[2 * (size_t)p + 1] = m2;
    out.samples[p] = n + n_samples;
  }
}

// ---- the decision --------------------------------------------------------------

constexpr uint32_t kTilesPerWg = kBlock / 64;  // a wave per tile

// One wave per shard tile, lane i its slot i: the lane forms its pixel's L and
// R (adapt_terms; +0 where the slot has no pixel), the wave sums each in the
// tree's order through LDS (adapt_tree_lane, the host's own step) and lane 0
// writes the tile's byte. only_running: a tile whose byte is already 0 left the
// running in an earlier round and stays as it is. At 64 values per tile nothing
// here is hot: a frame's tiles are a few thousand waves once per round.
__global__ __launch_bounds__(kBlock) void k_adaptive_tiles(AdaptFrame f, const float* moments,
                                                           const uint32_t* samples, float tau2, float floor,
                                                           uint8_t* open, uint32_t only_running, uint32_t* n_open) {
  __shared__ float sL[kTilesPerWg][kAdaptSlots], sR[kTilesPerWg][kAdaptSlots];
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t j = blockIdx.x * kTilesPerWg + wave;
  // wave-uniform; every wave of the workgroup still takes the barriers below
  const bool live = j < f.n_tiles && !(only_running && open[MRT_IDX(f, j, f.n_tiles, 33)] == 0);
  AdaptTerms t{0.0f, 0.0f};
  bool two = true;
  if (live) {
    const AdaptPixel px = adapt_pixel(f, j, lane);
    if (px.present) {
      const uint32_t p = MRT_IDX(f, px.p, f.W * f.H, 34);
      const uint32_t n = samples[p];
      t = adapt_terms(moments[2 * (size_t)p], moments[2 * (size_t)p + 1], n, tau2, floor);
      two = n >= 2;
    }
  }
  sL[wave][lane] = t.L;
  sR[wave][lane] = t.R;
  for (uint32_t k = kAdaptSlots / 2; k != 0; k /= 2) {
    __syncthreads();
    adapt_tree_lane(sL[wave], lane, k);
    adapt_tree_lane(sR[wave], lane, k);
  }
  __syncthreads();
  const bool all_two = __ballot(!two) == 0;
  if (live && lane == 0) {
    const bool closed = adapt_closed(all_two, sL[wave][0], sR[wave][0]);
    open[MRT_IDX(f, j, f.n_tiles, 33)] = closed ? 0 : 1;
    if (!closed && n_open) atomicAdd(n_open, 1u);  // a count: the order of arrival does not matter
  }
}

// ---- the next round's pixel list ---------------------------------------------

// The open tiles' pixels in shard_list's order (tiles in shard order, a tile's
// pixels in raster order = slot order), as a dense list: tile j's pixels start
// at the number of pixels of the open tiles before it. Three launches, no
// atomics and no hand-off between workgroups inside a launch, so the list is
// the same whatever the dispatch order:
//   k_adaptive_scan_tiles : per workgroup of kBlock tiles, each tile's offset
//       within the workgroup (shuffle scan within a wave, LDS across the waves)
//       and the workgroup's totals {pixels, open tiles};
//   k_adaptive_scan_blocks: one workgroup turns the totals into offsets (kBlock
//       at a time, carrying the sum) and writes the round's word {pixels, open
//       tiles} where the host reads it;
//   k_adaptive_compact    : one wave per open tile, lane i its slot i: the
//       present lanes' ranks (ballot + popcount prefix) behind the tile's
//       offset are the pixels' places.
// 2^26 tiles are 2^18 totals: 1024 trips of the one workgroup.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane_id() >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void k_adaptive_scan_tiles(AdaptFrame f, const uint8_t* open, uint32_t* tile_off,
                                                                uint2* block_sum, uint32_t n_blocks) {
  __shared__ uint32_t s_pix[kWaves], s_open[kWaves];
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  const bool is_open = j < f.n_tiles && open[MRT_IDX(f, j, f.n_tiles, 33)] != 0;
  const uint32_t c = is_open ? adapt_tile_pixels(f, j) : 0u;
  const uint32_t v = wave_scan_incl(c);
  const unsigned long long open_mask = __ballot(is_open);
  if (lane == 63) s_pix[wave] = v;
  if (lane == 0) s_open[wave] = (uint32_t)__popcll(open_mask);
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t w = 0; w < wave; ++w) base += s_pix[w];
  if (j < f.n_tiles) tile_off[MRT_IDX(f, j, f.n_tiles, 33)] = base + v - c;
  if (threadIdx.x == 0) {
    uint32_t pix = 0, op = 0;
    for (uint32_t w = 0; w < kWaves; ++w) pix += s_pix[w], op += s_open[w];
    block_sum[MRT_IDX(f, blockIdx.x, n_blocks, 35)] = make_uint2(pix, op);
  }
}

__global__ __launch_bounds__(kBlock) void k_adaptive_scan_blocks(uint2* block_sum, uint32_t n_blocks, AdaptWord* word,
                                                                 DbgRec D) {
  __shared__ uint32_t s_pix[kWaves], s_open[kWaves];
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  uint32_t carry_pix = 0, carry_open = 0;  // the same in every thread
  for (uint32_t b0 = 0; b0 < n_blocks; b0 += kBlock) {
    const uint32_t i = b0 + threadIdx.x;
    const uint2 s = i < n_blocks ? block_sum[MRT_IDX(D, i, n_blocks, 35)] : make_uint2(0u, 0u);
    const uint32_t v = wave_scan_incl(s.x);
    const uint32_t o = wave_sum(s.y);
    if (lane == 63) s_pix[wave] = v;
    if (lane == 0) s_open[wave] = o;
    __syncthreads();
    uint32_t base = 0, pix = 0, op = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
      if (w < wave) base += s_pix[w];
      pix += s_pix[w];
      op += s_open[w];
    }
    if (i < n_blocks) block_sum[MRT_IDX(D, i, n_blocks, 35)].x = carry_pix + base + v - s.x;
    carry_pix += pix;
    carry_open += op;
    __syncthreads();  // the next trip overwrites s_pix and s_open
  }
  if (threadIdx.x == 0) {
    *word = AdaptWord{carry_pix, carry_open};
    __threadfence_system();
  }
}

__global__ __launch_bounds__(kBlock) void k_adaptive_compact(AdaptFrame f, const uint8_t* open,
                                                             const uint32_t* tile_off, const uint2* block_sum,
                                                             uint32_t n_blocks, uint32_t* list, uint32_t list_cap) {
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t j = blockIdx.x * kTilesPerWg + wave;
  if (j >= f.n_tiles || open[MRT_IDX(f, j, f.n_tiles, 33)] == 0) return;  // wave-uniform; no barrier below
  const AdaptPixel px = adapt_pixel(f, j, lane);
  const unsigned long long mask = __ballot(px.present);
  const uint32_t pos = block_sum[MRT_IDX(f, j / kBlock, n_blocks, 35)].x + tile_off[MRT_IDX(f, j, f.n_tiles, 33)] +
                       lane_rank(mask);
  // pos < the open tiles' pixels <= the shard's pixels = list_cap by construction
  if (px.present && pos < list_cap) list[MRT_IDX(f, pos, list_cap, 36)] = px.p;
}

// ---- resolve -------------------------------------------------------------------

// out = (1.0f / (float)n) * sum per channel, k_tonemap's own scale * sum; zeros where n == 0.
__global__ __launch_bounds__(kBlock) void k_adaptive_resolve(const float* rgb, const uint32_t* samples, float* out,
                                                             uint32_t n_frame, DbgRec D) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < n_frame; p += (size_t)gridDim.x * kBlock) {
    const uint32_t q = MRT_IDX(D, (uint32_t)p, n_frame, 37);
    const uint32_t n = samples[q];
    const float scale = n ? 1.0f / (float)n : 0.0f;
#pragma unroll
    for (uint32_t ch = 0; ch < 3; ++ch) out[3 * (size_t)q + ch] = n ? scale * rgb[3 * (size_t)q + ch] : 0.0f;
  }
}

uint32_t scan_blocks(uint32_t n_tiles) { return (n_tiles + kBlock - 1) / kBlock; }

AdaptFrame checked_frame(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  check_image_size(W, H);
  if (sc == 0) sc = 1;
  if (si >= sc) throw ApiError{MRT_ERR_INVALID, "shard_index >= shard_count"};
  const AdaptFrame f = adapt_frame(W, H, si, sc, c ? c->dbg.p : nullptr);
  if (f.n_tiles > kAdaptMaxTiles) throw ApiError{MRT_ERR_INVALID, "adaptive: a shard of more than 2^26 tiles"};
  return f;
}

}  // namespace

// ---- what render.hip's rounds call ---------------------------------------------

void accumulate_moments(mrt_ctx* c, const RenderParams& rp, float* d_rgb, uint32_t* d_b, float* d_moments,
                        uint32_t* d_samples, hipStream_t st) {
  const MomOut out{d_rgb, d_b, d_moments, d_samples, rp.W * rp.H, c->dbg.p};
  hipLaunchKernelGGL(k_accumulate_moments, dim3((rp.n_pix + kMomPix - 1) / kMomPix), dim3(kBlock), 0, st,
                     (const float4*)c->results.p, rp.n_pix, rp.spp, rp.pixlist, out);
  HIP_CHECK(hipGetLastError());
}

AdaptFrame adaptive_frame(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  return checked_frame(c, W, H, si, sc);
}

// The context's scratch for a shard of n_tiles tiles and n_pix pixels: the
// tiles' bytes, the scan's words, the two lists. It grows on demand; a call
// returns only when its kernels have ended, so nothing of this context still
// reads the old buffers, and the synchronisation covers a caller who shares
// them in ways the header does not allow for.
void adaptive_scratch(mrt_ctx* c, uint32_t n_tiles, uint32_t n_pix) {
  if (!c->ad_words_h) {
    HIP_CHECK(hipHostMalloc(&c->ad_words_h, kAdaptMaxRounds * sizeof(AdaptWord),
                            hipHostMallocCoherent | hipHostMallocMapped));
    memset(c->ad_words_h, 0, kAdaptMaxRounds * sizeof(AdaptWord));
    HIP_CHECK(hipHostGetDevicePointer((void**)&c->ad_words_d, c->ad_words_h, 0));
    HIP_CHECK(hipEventCreateWithFlags(&c->ad_ev, hipEventDisableTiming));
  }
  // an offset per tile, a pad word to the totals' 8-byte boundary, two words per kBlock tiles (adaptive_compact)
  const size_t scan_words = (size_t)n_tiles + 1 + 2 * (size_t)scan_blocks(n_tiles);
  if (c->ad_open.n >= n_tiles && c->ad_scan.n >= scan_words && c->ad_list[0].n >= n_pix && c->ad_list[1].n >= n_pix)
    return;
  if (c->ad_open.p) HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(c->ad_open.reserve(n_tiles));
  HIP_CHECK(c->ad_scan.reserve(scan_words));
  HIP_CHECK(c->ad_list[0].reserve(n_pix));
  HIP_CHECK(c->ad_list[1].reserve(n_pix));
}

void adaptive_evaluate(const AdaptFrame& f, const float* d_moments, const uint32_t* d_samples, float tau2, float floor,
                       uint8_t* d_open, bool only_running, uint32_t* d_n_open, hipStream_t st) {
  if (f.n_tiles == 0) return;
  hipLaunchKernelGGL(k_adaptive_tiles, dim3((f.n_tiles + kTilesPerWg - 1) / kTilesPerWg), dim3(kBlock), 0, st, f,
                     d_moments, d_samples, tau2, floor, d_open, only_running ? 1u : 0u, d_n_open);
  HIP_CHECK(hipGetLastError());
}

// The open tiles of c->ad_open -> `list` (capacity list_cap) and round
// `round`'s word; waits for the word and returns it.
AdaptWord adaptive_compact(mrt_ctx* c, const AdaptFrame& f, uint32_t* list, uint32_t list_cap, uint32_t round,
                           hipStream_t st) {
  const uint32_t nb = scan_blocks(f.n_tiles);
  uint32_t* tile_off = c->ad_scan.p;
  // the totals behind the tile offsets, on an 8-byte boundary
  uint2* block_sum = (uint2*)(c->ad_scan.p + ((size_t)f.n_tiles + 1) / 2 * 2);
  AdaptWord* word = c->ad_words_d + round;
  hipLaunchKernelGGL(k_adaptive_scan_tiles, dim3(nb), dim3(kBlock), 0, st, f, (const uint8_t*)c->ad_open.p, tile_off,
                     block_sum, nb);
  hipLaunchKernelGGL(k_adaptive_scan_blocks, dim3(1), dim3(kBlock), 0, st, block_sum, nb, word, DbgRec{c->dbg.p});
  hipLaunchKernelGGL(k_adaptive_compact, dim3((f.n_tiles + kTilesPerWg - 1) / kTilesPerWg), dim3(kBlock), 0, st, f,
                     (const uint8_t*)c->ad_open.p, (const uint32_t*)tile_off, (const uint2*)block_sum, nb, list,
                     list_cap);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(c->ad_ev, st));
  HIP_CHECK(hipEventSynchronize(c->ad_ev));
  const volatile AdaptWord& v = c->ad_words_h[round];  // written by the GPU
  return AdaptWord{v.pixels, v.tiles};
}

extern "C" {

int mrt_adaptive_default_params(mrt_adaptive_params* out) {
  if (!out) {
    mrt_global_error = "null output";
    return MRT_ERR_INVALID;
  }
  // a step of 128: every round pays a fill and a drain of the wavefront loop, 30-70 ms at 1920x1080 whatever the
  // step (DESIGN.md "Adaptive sampling": step 16 ran 1.7-3.4x the uniform render's time with nothing stopping)
  *out = mrt_adaptive_params{16u, 128u, 0.05f, 0.01f};
  return MRT_OK;
}

int mrt_adaptive_tiles(uint32_t W, uint32_t H, uint32_t si, uint32_t sc, const float* moments, const uint32_t* samples,
                       const mrt_adaptive_params* params, uint8_t* open, uint32_t* n_open) {
  try {
    if (const char* why = adapt_params_error(params)) throw ApiError{MRT_ERR_INVALID, why};
    if (!moments || !samples || !open) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const AdaptFrame f = checked_frame(nullptr, W, H, si, sc);
    const float tau2 = adapt_tau2(params->threshold);
    uint32_t n = 0;
    for (uint32_t j = 0; j < f.n_tiles; ++j) {
      open[j] = adapt_tile_open(f, j, moments, samples, tau2, params->floor) ? 1 : 0;
      n += open[j];
    }
    if (n_open) *n_open = n;
    return MRT_OK;
  } catch (const ApiError& e) {
    mrt_global_error = e.msg;
    return e.code;
  }
}

int mrt_adaptive_tiles_device(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc, const float* d_moments,
                              const uint32_t* d_samples, const mrt_adaptive_params* params, uint8_t* d_open,
                              uint32_t* d_n_open, void* stream) {
  MRT_DEV0(c, mrt_adaptive_tiles_device(c, W, H, si, sc, d_moments, d_samples, params, d_open, d_n_open, stream));
  return guarded(c, [&] {
    if (const char* why = adapt_params_error(params)) throw ApiError{MRT_ERR_INVALID, why};
    if (!d_moments || !d_samples || !d_open) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const AdaptFrame f = checked_frame(c, W, H, si, sc);
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream
    if (d_n_open) HIP_CHECK(hipMemsetAsync(d_n_open, 0, 4, st));
    adaptive_evaluate(f, d_moments, d_samples, adapt_tau2(params->threshold), params->floor, d_open, false, d_n_open,
                      st);
  });
}

int mrt_adaptive_resolve_device(mrt_ctx* c, uint32_t W, uint32_t H, const float* d_rgb, const uint32_t* d_samples,
                                float* d_out, void* stream) {
  MRT_DEV0(c, mrt_adaptive_resolve_device(c, W, H, d_rgb, d_samples, d_out, stream));
  return guarded(c, [&] {
    check_image_size(W, H);
    if (!d_rgb || !d_samples || !d_out) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const uint32_t n = W * H;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + kBlock - 1) / kBlock, 1u << 20);
    hipLaunchKernelGGL(k_adaptive_resolve, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, d_rgb, d_samples, d_out, n,
                       DbgRec{c->dbg.p});
    HIP_CHECK(hipGetLastError());
  });
}

int mrt_adaptive_resolve(mrt_ctx* c, uint32_t W, uint32_t H, const float* rgb, const uint32_t* samples, float* out) {
  MRT_DEV0(c, mrt_adaptive_resolve(c, W, H, rgb, samples, out));
  return guarded(c, [&] {
    check_image_size(W, H);
    if (!rgb || !samples || !out) throw ApiError{MRT_ERR_INVALID, "null buffer"};
    const size_t n = (size_t)W * H;
    DevBuf<float> d;
    DevBuf<uint32_t> dn;
    HIP_CHECK(d.alloc(6 * n));
    HIP_CHECK(dn.alloc(n));
    HIP_CHECK(hipMemcpyAsync(d.p, rgb, n * 12, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(dn.p, samples, n * 4, hipMemcpyHostToDevice, c->stream));
    const int rc = mrt_adaptive_resolve_device(c, W, H, d.p, dn.p, d.p + 3 * n, c->stream);
    if (rc != MRT_OK) throw ApiError{rc, c->err};
    HIP_CHECK(hipMemcpyAsync(out, d.p + 3 * n, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
  });
}

}  // extern "C"
