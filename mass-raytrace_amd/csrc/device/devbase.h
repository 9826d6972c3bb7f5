// devbase.h — what the device headers share: the function qualifiers,
// primitive references, the counters, checked scene-array indices, bit casts.
// MRT_HD (mrt_math.h) marks what a single ray's traversal executes: the same
// source runs on the host (tools/slab_check.cpp drives it there), bit for bit
// — every operation a correctly rounded IEEE one in a fixed order; build with
// -ffp-contract=off and correctly rounded f32 divide/sqrt. MRT_DEV is the rest.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MRT_DEV __device__ __forceinline__
#else
// A plain C++ compiler (a host tool built without hipcc): the two vector types
// the records and the ray pool are made of; MRT_DEV code is parsed, never run.
struct alignas(16) uint4 {
  uint32_t x, y, z, w;
};
struct alignas(16) float4 {
  float x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
#define __shared__
#define MRT_DEV inline
#endif

#include "../../../include/massrt.h"
#include "../mrt_math.h"
#include "layout.h"

namespace mrt {

constexpr uint32_t kRefNone = 0u;
MRT_HD uint32_t make_ref(uint32_t kind, uint32_t idx) { return (kind << 28) | idx; }

struct DevCounters {
  unsigned long long samples, segments, node_visits, sphere_tests, triangle_tests, instance_entries,
      model_entries, closest_hits, texel_taps, bounces, wave_slots, lane_steps, box_exact, shaded, vnf_fallbacks,
      shade_waves, shade_kinds, shade_materials;
};

struct LocalCounters {
  uint32_t node_visits = 0, sphere_tests = 0, triangle_tests = 0, instance_entries = 0, model_entries = 0,
           texel_taps = 0, wave_slots = 0, lane_steps = 0, box_exact = 0, vnf_fallbacks = 0, shade_waves = 0,
           shade_kinds = 0, shade_materials = 0;
};

// Bounds checks of every scene-array index, compiled in with
// -DMRT_DEBUG_BOUNDS (libmassrt_dbg.so): a failing index is recorded in
// S.dbg and replaced by 0, so a bad index shows up as a record instead of a
// GPU memory fault. On the host a failing index is printed and the program
// aborts.
#ifdef MRT_DEBUG_BOUNDS
MRT_HD uint32_t mrt_chk(uint32_t* dbg, uint32_t idx, uint32_t bound, uint32_t code) {
  if (idx < bound) return idx;
#if defined(__HIP_DEVICE_COMPILE__)
  if (atomicCAS(dbg, 0u, code) == 0u) {
    dbg[1] = idx;
    dbg[2] = bound;
  }
  atomicAdd(dbg + 3, 1u);
  return 0;
#else
  fprintf(stderr, "index out of bounds: check %u, index %u, bound %u\n", code, idx, bound);
  abort();
#endif
}
#define MRT_IDX(S, idx, bound, code) mrt_chk((S).dbg, (idx), (bound), (code))
#else
#define MRT_IDX(S, idx, bound, code) (idx)
#endif

MRT_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
MRT_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
MRT_HD V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
// `c ? uv : V2{0, 0}` per component: the conditional on whole aggregates made
// clang select between the addresses of two stack temporaries, which kept
// them in scratch memory (k_shade spilled 44 B per lane)
MRT_HD V2 uv_or_zero(bool c, V2 uv) { return V2{c ? uv.x : 0.0f, c ? uv.y : 0.0f}; }

}  // namespace mrt
