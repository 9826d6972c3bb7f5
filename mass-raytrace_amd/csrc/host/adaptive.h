// adaptive.h — the arithmetic of mrt_render_adaptive (include/massrt.h states
// the rule): a pixel's two terms, a tile's slots and the order its 64 terms are
// summed in, the tiles of a shard, the round schedule and the argument checks.
// Plain C++, no HIP: the kernels (device/adaptive.hip), mrt_adaptive_tiles and
// the host loop (device/render.hip) all call these same functions, and
// tools/adaptive_check.cpp runs the schedule and the checks on the host
// (tests/test_adaptive.py). IEEE f32, + - * and comparisons only, in the order
// written; build uncontracted (-ffp-contract=off).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/massrt.h"
#include "../mrt_math.h"

namespace mrt {

constexpr uint32_t kAdaptSlots = MRT_TILE * MRT_TILE;
static_assert(kAdaptSlots == 64, "k_adaptive_tiles: one wave per tile, one lane per slot");
constexpr uint32_t kAdaptMaxRounds = 4096;
constexpr uint32_t kAdaptMaxTiles = 1u << 26;  // of one shard (k_adaptive_compact's scan)

// ---- the tiles of a shard ---------------------------------------------------

// The frame and the shard a call works on: shard tile j is frame tile
// si + j sc (loop.h shard_list's order), n_tiles of them.
struct AdaptFrame {
  uint32_t W, H, si, sc, n_tiles;
  uint32_t* dbg;  // MRT_IDX's record (DevScene::dbg); unused on the host
};

MRT_HD uint32_t adapt_tiles_x(uint32_t W) { return (W + MRT_TILE - 1) / MRT_TILE; }
// W H < 2^32: the product of the two tile counts fits 32 bits as well
MRT_HD uint32_t adapt_frame_tiles(uint32_t W, uint32_t H) { return adapt_tiles_x(W) * adapt_tiles_x(H); }
MRT_HD uint32_t adapt_shard_tiles(uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  const uint32_t t = adapt_frame_tiles(W, H);
  return t > si ? (uint32_t)(((uint64_t)(t - si) + sc - 1) / sc) : 0u;
}
inline AdaptFrame adapt_frame(uint32_t W, uint32_t H, uint32_t si, uint32_t sc, uint32_t* dbg = nullptr) {
  return AdaptFrame{W, H, si, sc, adapt_shard_tiles(W, H, si, sc), dbg};
}

// Slot i = (y % 8) * 8 + (x % 8) of a pixel, and back: the pixel of slot i of
// shard tile j. !present: the tile hangs over the frame's edge there.
MRT_HD uint32_t adapt_slot(uint32_t x, uint32_t y) { return (y % MRT_TILE) * MRT_TILE + (x % MRT_TILE); }
struct AdaptPixel {
  uint32_t p;
  bool present;
};
MRT_HD AdaptPixel adapt_pixel(const AdaptFrame& f, uint32_t j, uint32_t i) {
  const uint32_t t = f.si + j * f.sc, tx = adapt_tiles_x(f.W);
  const uint32_t x = (t % tx) * MRT_TILE + i % MRT_TILE, y = (t / tx) * MRT_TILE + i / MRT_TILE;
  const bool present = x < f.W && y < f.H;
  return AdaptPixel{present ? y * f.W + x : 0u, present};
}
// Pixels of shard tile j (edge tiles hold fewer than 64).
MRT_HD uint32_t adapt_tile_pixels(const AdaptFrame& f, uint32_t j) {
  const uint32_t t = f.si + j * f.sc, tx = adapt_tiles_x(f.W);
  const uint32_t bx = (t % tx) * MRT_TILE, by = (t / tx) * MRT_TILE;
  const uint32_t w = f.W - bx < MRT_TILE ? f.W - bx : MRT_TILE, h = f.H - by < MRT_TILE ? f.H - by : MRT_TILE;
  return w * h;
}

// ---- the decision -----------------------------------------------------------

// What a sample of colour (r, g, b) adds to its pixel's {m1, m2}: y and y y.
MRT_HD float adapt_luma(float r, float g, float b) { return (r + g) + b; }

// A pixel's two terms from its moments and count; a slot without a pixel
// contributes {+0, +0}.
struct AdaptTerms {
  float L, R;
};
MRT_HD AdaptTerms adapt_terms(float m1, float m2, uint32_t n, float tau2, float floor) {
  const float nf = (float)n;
  const float L = nf * m2 - m1 * m1;
  const float q = m1 + nf * floor;
  const float R = (tau2 * (nf - 1.0f)) * (q * q);
  return AdaptTerms{L, R};
}
MRT_HD float adapt_tau2(float threshold) { return threshold * threshold; }

// The sum of a tile's 64 values: for k = 32, 16, .., 1: v[i] = v[i] + v[i + k],
// i < k. adapt_tree_lane is lane i's part of step k: a wave runs the 64 lanes
// of a step at once (a barrier between steps), the host one after the other.
MRT_HD void adapt_tree_lane(float* v, uint32_t i, uint32_t k) {
  if (i < k) v[i] = v[i] + v[i + k];
}
inline float adapt_tree_sum(float* v) {
  for (uint32_t k = kAdaptSlots / 2; k != 0; k /= 2)
    for (uint32_t i = 0; i < k; ++i) adapt_tree_lane(v, i, k);
  return v[0];
}

// Closed: every present pixel has two samples and the summed terms compare; a
// NaN on either side leaves the tile open.
MRT_HD bool adapt_closed(bool all_two, float L_sum, float R_sum) { return all_two && L_sum <= R_sum; }

// The decision for shard tile j on the host: true = open.
inline bool adapt_tile_open(const AdaptFrame& f, uint32_t j, const float* moments, const uint32_t* samples, float tau2,
                            float floor) {
  float L[kAdaptSlots], R[kAdaptSlots];
  bool all_two = true;
  for (uint32_t i = 0; i < kAdaptSlots; ++i) {
    const AdaptPixel px = adapt_pixel(f, j, i);
    AdaptTerms t{0.0f, 0.0f};
    if (px.present) {
      const uint32_t n = samples[px.p];
      t = adapt_terms(moments[2 * (size_t)px.p], moments[2 * (size_t)px.p + 1], n, tau2, floor);
      all_two = all_two && n >= 2;
    }
    L[i] = t.L;
    R[i] = t.R;
  }
  const float ls = adapt_tree_sum(L), rs = adapt_tree_sum(R);
  return !adapt_closed(all_two, ls, rs);
}

// ---- the rounds -------------------------------------------------------------

// Samples per pixel round `round` adds to the open tiles, `done` of the cap
// given so far in this call: round 0 the minimum, every later round a step or
// what is left of the cap. Its sample indices are [spp_begin + done,
// spp_begin + done + count): they depend on the round alone.
MRT_HD uint32_t adapt_round_count(const mrt_adaptive_params& p, uint32_t cap, uint32_t round, uint32_t done) {
  if (round == 0) return p.min_spp;
  const uint32_t left = cap - done;
  return p.step_spp < left ? p.step_spp : left;
}
// Rounds a call runs at most (every tile open to the end); min_spp <= cap, step_spp > 0.
inline uint64_t adapt_round_limit(const mrt_adaptive_params& p, uint32_t cap) {
  return 1 + ((uint64_t)(cap - p.min_spp) + p.step_spp - 1) / p.step_spp;
}
// After round `round`'s evaluation: does the call go on?
MRT_HD bool adapt_goes_on(uint32_t tiles_open, uint32_t done, uint32_t cap) { return tiles_open != 0 && done < cap; }

// ---- the argument checks ----------------------------------------------------

inline bool adapt_finite_nonneg(float x) { return x >= 0.0f && x <= 3.4028234663852886e38f; }  // NaN: false

// What is wrong with the rule's parameters alone (mrt_adaptive_tiles); nullptr: nothing.
inline const char* adapt_params_error(const mrt_adaptive_params* p) {
  if (!p) return "null adaptive params";
  if (!adapt_finite_nonneg(p->threshold)) return "adaptive: threshold must be finite and >= 0";
  if (!adapt_finite_nonneg(p->floor)) return "adaptive: floor must be finite and >= 0";
  return nullptr;
}
// ... and with them for a render of samples [spp_begin, spp_begin + spp_count).
inline const char* adapt_render_error(const mrt_adaptive_params* p, uint32_t spp_begin, uint32_t spp_count,
                                      uint32_t flags) {
  if (const char* why = adapt_params_error(p)) return why;
  if (p->step_spp == 0) return "adaptive: step_spp must be at least 1";
  if (p->min_spp > spp_count) return "adaptive: min_spp is above the cap (spp_count)";
  if (adapt_round_limit(*p, spp_count) > kAdaptMaxRounds) return "adaptive: more than 4096 rounds";
  if (flags & (MRT_RENDER_FUSED | MRT_RENDER_SIMPLE_TRACE))
    return "adaptive: MRT_RENDER_FUSED and MRT_RENDER_SIMPLE_TRACE render whole frames";
  if ((uint64_t)spp_begin + spp_count > 0xFFFFFFFFull) return "sample index overflow";
  return nullptr;
}

}  // namespace mrt
