// pool.h — the wavefront loop's device-side state (path pool, control words,
// per-chunk parameters) and the wave / workgroup helpers its kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../host/loop.h"
#include "path.h"

constexpr int kBlock = 256;

// XCD groups: workgroups are dealt round-robin over the 8 XCDs, so
// blockIdx.x % 8 names the workgroups that share one XCD's L2.
constexpr uint32_t kGroups = 8;
struct Ctrl {
  uint32_t active[2];
  uint32_t next_work;
  uint32_t shade_short;  // nonzero: a k_shade grid did not cover its live pool (host bound wrong; reported)
  // shade_bin 2: the survivors of the first half of the keys counted from the
  // bottom of the next pool (low word) and of the second half from its top
  // (high word), in one 64-bit word so that a workgroup reserves both with
  // ONE atomic (two, one per word, doubled k_shade's solo time: every
  // workgroup's atomics go to this one line)
  unsigned long long surv[2];
  // refill (k_reserve -> k_refill): work items [gen_base, gen_base + gen_count)
  // go to pool slots [gen_slot, gen_slot + gen_count), behind the survivors
  uint32_t gen_slot, gen_count, gen_base;
  // shade_bin 2: k_reserve closes the gap between the pool's two ends that
  // the refill leaves: k_refill moves gen_move paths from gen_move_src.. to
  // gen_move_dst..
  uint32_t gen_move, gen_move_src, gen_move_dst;
  uint32_t pad_[18];
  // persistent k_trace work counters (zeroed by k_shade), one 128-B line per
  // XCD group: group g takes its rays from the g-th eighth of the pool
  uint32_t group_next[kGroups * 32];
};
// The Ctrl a launch sequence starts from (copied to the device): pool 0 holds
// `active0` paths, everything else zero but next_work, k_render's work counter
// (mrt_trace_rays starts it at its ray count: none is left to hand out).
inline Ctrl ctrl_init(uint32_t active0, uint32_t next_work = 0) { return Ctrl{{active0, 0}, next_work, 0}; }

// SoA path state, 5 x 16 B per slot:
//   ro  = {o.x, o.y, o.z, work index g}    rd  = {d.x, d.y, d.z, bounces k}
//   thr = {T.x, T.y, T.z, kHoldsL or 0}    rad = {L.x, L.y, L.z, -}
//   rng = xoroshiro128** {s0.lo, s0.hi, s1.lo, s1.hi}
// rad is read and written only while thr.w says the path holds radiance
// (some component of L has nonzero bits): a path gains L only where a hit
// both emits and scatters (a Mix of DiffuseLight and a scattering material)
// — most paths end where they first gain it — so the slot's rad is
// otherwise stale and L is +0.
struct PathBufs {
  float4* ro;
  float4* rd;
  float4* thr;
  float4* rad;
  uint4* rng;
};

struct RenderParams {
  uint32_t W, H;
  unsigned long long seed;
  uint32_t max_depth;
  uint32_t n_pix;        // pixels in this shard
  uint32_t G;            // work items in this chunk = n_pix * spp
  uint32_t spp;          // samples per pixel in this chunk
  uint32_t sample_base;  // absolute sample index of chunk sample 0
  uint32_t pool_cap;     // path slots per buffer
  const uint32_t* pixlist;
  uint32_t shade_bin;    // k_shade: survivors grouped by material kind and direction in the next pool (option shade_bin)
};

// One view of a batch (mrt_render_views): its camera and the seed of its
// samples' streams. The context keeps the batch's table on the device; the
// kernels only read it.
struct alignas(16) DevView {
  mrt::DevCamera cam;
  uint32_t pad_;
  unsigned long long seed;
};
static_assert(sizeof(DevView) == 96 && offsetof(DevView, seed) == 80, "DevView: 96 B, the seed on an 8-B boundary");

// Where k_generate<ViewTable> / k_refill<ViewTable> take the camera from: the
// render's pixel list then holds global pixels P = v pix_per_view + p
// (loop.h view_split). Its own kernel argument; RenderParams stays as it is.
struct ViewTable {
  const DevView* views;
  uint32_t pix_per_view;  // W H
  uint32_t n_views;
  uint32_t* dbg;  // MRT_IDX's record (DevScene::dbg)
};

// Where k_generate<RayTable> / k_refill<RayTable> take a path's start from
// (mrt_render_rays): work item g = i spp + s is sample s of entry i (loop.h
// ray_work), its result goes to list position i. Entries are 32 B, read as two
// 16-byte loads: the table is 16-byte aligned. The kernels only read it.
struct RayTable {
  const mrt_path_ray* rays;
  uint32_t n;
  uint32_t* dbg;  // MRT_IDX's record (DevScene::dbg)
};
static_assert(sizeof(mrt_path_ray) == 32 && offsetof(mrt_path_ray, key) == 24 && offsetof(mrt_path_ray, skip) == 28,
              "mrt_path_ray: two quads, {o, d.x} {d.y, d.z, key, skip}");
static_assert(mrt::kRaySkipMax == MRT_RAY_SKIP_MAX, "loop.h ray_skip clamps to the ABI's limit");

constexpr float kTmin = 0.001f;         // World::intersect(ray, 0.001, INFINITY) (main.rs trace)
constexpr uint32_t kIdle = 0xFFFFFFFFu;  // Trav.ray of a lane without a ray

namespace {

constexpr uint32_t kHoldsL = 1u;
__device__ __forceinline__ bool holds_l(const float4& thr) { return __float_as_uint(thr.w) != 0u; }
__device__ __forceinline__ bool nonzero_bits(float x, float y, float z) {
  return (__float_as_uint(x) | __float_as_uint(y) | __float_as_uint(z)) != 0u;
}

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }
__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

constexpr uint32_t kWaves = kBlock / 64;

// Workgroup-wide reservation of `count` (this wave's share) consecutive
// slots from *counter: one atomic per workgroup; returns this wave's first
// slot. Every thread of the workgroup must call it.
template <uint32_t NW = kWaves>
__device__ __forceinline__ uint32_t wg_reserve(uint32_t* counter, uint32_t count, uint32_t wave, uint32_t* s_cnt,
                                               uint32_t& s_base) {
  if (lane_id() == 0) s_cnt[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) total += s_cnt[w];
    s_base = total ? atomicAdd(counter, total) : 0u;
  }
  __syncthreads();
  uint32_t base = s_base;
  for (uint32_t w = 0; w < wave; ++w) base += s_cnt[w];
  __syncthreads();  // s_cnt/s_base are reused by the next call
  return base;
}

// wg_reserve for the alive lanes, the workgroup's survivors ordered by `key`
// (< kOutKeys): a lane's rank within its key comes from an LDS atomic (so
// the order within a key is arbitrary — paths are independent, the images
// do not depend on it), the keys' offsets from one wave's scan of the
// histogram. k_shade uses it to group the next pool's rays by the material
// kind they scattered from and the signs of their direction's y and x
// (option shade_bin): k_trace's waves then walk rays that go the same way
// together (round 5, profiles/r5_shade_bin/: kind only 1003 / 514, octant
// 1018 / 526, kind x octant 1022 / 528, y sign only 1038 / 531, kind x y x x
// 1035 / 535 Msamples/s on sphere_grid / cube_field, none 974 / 504). Every
// thread of the workgroup must call it.
constexpr uint32_t kOutKeys = 64;  // one wave scans the histogram (k_shade's keys use 32)
// hi != nullptr (shade_bin 2): keys >= 32 take slots counted down from the
// top of the pool (cap - 1, cap - 2, ...) instead: both counts go to *hi
// (low word: from the bottom, high word: from the top, one atomic; *counter
// is unused), the next pool then holds the two halves at its two ends, and
// k_reserve/k_refill put the new camera rays between them.
__device__ __forceinline__ uint32_t wg_reserve_keyed(uint32_t* counter, bool alive, uint32_t key, uint32_t* s_hist,
                                                     unsigned long long* hi = nullptr, uint32_t cap = 0) {
  if (threadIdx.x < kOutKeys) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t rank = alive ? atomicAdd(&s_hist[key], 1u) : 0u;
  __syncthreads();
  if (threadIdx.x < kOutKeys) {  // wave 0: exclusive scan of the 64 counts
    const uint32_t c = s_hist[threadIdx.x];
    uint32_t v = c;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(v, d, 64);
      if (lane_id() >= d) v += u;
    }
    const uint32_t total = __shfl(v, 63, 64);
    const uint32_t tlo = hi ? __shfl(v, 31, 64) : total, thi = total - tlo;
    uint32_t b = 0, bh = 0;
    if (threadIdx.x == 0) {
      if (hi) {
        const unsigned long long r = total ? atomicAdd(hi, ((unsigned long long)thi << 32) | tlo) : 0ull;
        b = (uint32_t)r;
        bh = (uint32_t)(r >> 32);
      } else {
        b = total ? atomicAdd(counter, total) : 0u;
      }
    }
    b = __shfl(b, 0, 64);
    bh = __shfl(bh, 0, 64);
    s_hist[threadIdx.x] = hi && threadIdx.x >= 32 ? cap - 1u - bh - (v - c - tlo) : b + v - c;
  }
  __syncthreads();
  const uint32_t slot = hi && key >= 32 ? s_hist[key] - rank : s_hist[key] + rank;
  __syncthreads();  // s_hist is reused by the next call
  return slot;
}

__device__ void flush_counters(mrt::DevCounters* c, const mrt::LocalCounters& lc, uint32_t segs, uint32_t hits,
                               uint32_t samples, uint32_t bounces, uint32_t shaded = 0) {
  uint32_t v[18] = {samples,         segs,           lc.node_visits, lc.sphere_tests,   lc.triangle_tests, lc.instance_entries,
                    lc.model_entries, hits,           lc.texel_taps,  bounces,           lc.wave_slots,     lc.lane_steps,
                    lc.box_exact,     shaded,         lc.vnf_fallbacks, lc.shade_waves, lc.shade_kinds,    lc.shade_materials};
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(c);
#pragma unroll
  for (int k = 0; k < 18; ++k) {
    uint32_t s = wave_sum(v[k]);
    if (lane_id() == 0 && s) atomicAdd(dst + k, (unsigned long long)s);
  }
}

}  // namespace
