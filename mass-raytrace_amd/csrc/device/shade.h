// shade.h — one shading step of a path, shared by k_shade and k_render
// (render.hip).
#pragma once
#include "pool.h"

namespace {

using namespace mrt;

// One level of main.rs trace() after World::intersect returned `h` for the
// ray (o, d): adds T * emitted (hit) or T * background (miss) to L; on a
// scatter that continues (and depth left) moves (o, d) to the scattered ray,
// multiplies T by the attenuation and returns true.
// (mat: the hit's material index, kShadeMiss for a miss: the counting
// k_shade's coherence counters; mkind: that material's own kind — a Mix's is
// Mix, not the picked leaf's — from the record scatter() fetched: k_shade's
// survivor key)
constexpr uint32_t kShadeMiss = 0xFFFFFFFEu, kShadeIdle = 0xFFFFFFFFu;
template <bool EXT>
MRT_DEV bool shade_step(const DevScene& S, uint32_t max_depth, const Hit& h, V3& o, V3& d, V3& T, V3& L, uint32_t& k,
                        PathRng& rng, LocalCounters& lc, uint32_t& nbounce, uint32_t& mat, uint32_t& mkind) {
  if (h.prim == kRefNone) {
    mat = kShadeMiss;
    L = L + T * background<EXT>(S, d, lc);
    return false;
  }
  Surf s = resolve_hit<EXT>(S, o, d, h, lc);
  mat = s.material;
  V3 emitted, atten, nd;
  bool cont = scatter<EXT>(S, s, d, rng, emitted, atten, nd, lc, mkind);
  L = L + T * emitted;
  if (!cont) return false;
  T = T * atten;
  k += 1;
  nbounce += 1;
  o = s.point;
  d = nd;
  return k < max_depth;  // trace(depth 0) returns (0, 0)
}

// How coherent a k_shade wave's shading is (counting launches only; SURVEY
// §7 step 7 asks whether sorting rays by material would pay): per wave with
// work, the distinct material kinds among its lanes (a miss counts as one
// more kind: the background branch) — the branches the wave executes one
// after another — and the distinct material indices (the material records
// it gathers). A material-sorted pool could bring both to ~1.
MRT_DEV void shade_coherence(uint32_t mat, uint32_t mkind, LocalCounters& lc) {
  const unsigned long long act = __ballot(mat != kShadeIdle);
  if (act == 0) return;
  const uint32_t kind = mat == kShadeIdle ? 0xFFu : mat == kShadeMiss ? 16u : mkind;
  uint32_t nk = 0, nm = 0;
  for (uint32_t kk = 0; kk <= 16; ++kk) nk += __ballot(kind == kk) != 0;
  for (unsigned long long rem = act; rem;) {
    const uint32_t m0 = __shfl(mat, __ffsll((long long)rem) - 1, 64);
    rem &= ~__ballot(mat == m0);
    ++nm;
  }
  if (lane_id() == 0) {
    lc.shade_waves += 1;
    lc.shade_kinds += nk;
    lc.shade_materials += nm;
  }
}

}  // namespace
